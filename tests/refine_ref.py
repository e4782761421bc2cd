"""The definition of the exact re-rank (include/nlsh_hip.h, nlsh_rerank_topk) in numpy.

`pair_bits` is the reference for the distance of a (query, row) pair: the tiled float32 scan's own bits, taken from float32 twin indexes
over the ORIGINAL rows whose bucket keys are all zero -- one bucket of at most 256 rows per twin (more rows: one twin per 256-row chunk,
as tests/test_gpu_range_query.py cuts its twin), scanned with k = rows of the chunk, so every (query, row) pair is scored and returned.
For L2 the table is also held against `oracle.distances`, bit for bit.  `rerank_reference` selects by sort key as the definition says.
Neither calls the code under test."""
import numpy as np
import torch

CHUNK = 256


def mono_u32(bits_u32):
    """float32 bits -> the uint32 whose unsigned order is the float order (csrc/common.h, mono_from_float)."""
    u = np.asarray(bits_u32, dtype=np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _distance(metric):
    from nlsh_amd.data import Glove, SIFT
    return SIFT.distance if metric == "l2" else Glove.distance


def pair_bits(rows, queries, metric, hashing, check_oracle=True):
    """rows float32 [N, d], queries float32 [Q, d] (numpy) -> float32 [Q, N]: the tiled float32 scan's distance of every pair."""
    from nlsh_amd.indexer import Indexer
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    N, Q = rows.shape[0], queries.shape[0]
    out = np.full((Q, N), np.nan, dtype=np.float32)
    seen = np.zeros((Q, N), dtype=bool)
    qd = torch.from_numpy(queries).cuda()
    keys = torch.zeros((Q, 1), dtype=torch.int32, device="cuda")
    nkeys = torch.ones((Q,), dtype=torch.int32, device="cuda")
    for lo in range(0, N, CHUNK):
        part = rows[lo:lo + CHUNK]
        n = part.shape[0]
        twin = Indexer(hashing, torch.from_numpy(part).cuda(), _distance(metric), compat=False, algo="tiled", id_base=lo,
                       corpus_keys=torch.zeros((n,), dtype=torch.int32, device="cuda"))
        dist, idx, nc, _ = twin.scan_tensors(qd, keys, nkeys, k=n)
        assert bool((nc == n).all())
        dist, idx = dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
        assert np.array_equal(np.sort(idx, axis=1), np.tile(np.arange(lo, lo + n), (Q, 1))), "the twin returned every row once"
        np.put_along_axis(out, idx, dist, axis=1)
        np.put_along_axis(seen, idx, True, axis=1)
    assert seen.all()
    if check_oracle and metric == "l2":
        from oracle import oracle
        ids = np.arange(N, dtype=np.int32)
        for q in range(Q):
            assert np.array_equal(oracle.distances(queries[q], rows, ids, "l2").view(np.uint32), out[q].view(np.uint32)), q
    return out


def rerank_reference(bits, cand, k, id_base=0):
    """bits float32 [Q, N] (`pair_bits`; column = id - id_base), cand int [Q, kc] -> (dist float32 [Q, k], idx int32 [Q, k],
    keys uint64 [Q, k], count int32 [Q], first_bad int): per query the k smallest  mono(dist) << 32 | id  over the valid ids of its list,
    ascending, padded with +inf / -1 / ~0.  -1 is padding; any other id outside [id_base, id_base + N) is dropped and reported."""
    bits = np.asarray(bits, dtype=np.float32)
    cand = np.asarray(cand, dtype=np.int64)
    Q, N = bits.shape
    dist = np.full((Q, k), np.inf, dtype=np.float32)
    idx = np.full((Q, k), -1, dtype=np.int32)
    keys = np.full((Q, k), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    count = np.zeros((Q,), dtype=np.int32)
    first_bad = -1
    for q in range(Q):
        ids = cand[q]
        rel = ids - id_base
        valid = (ids != -1) & (rel >= 0) & (rel < N)
        if ((ids != -1) & ~valid).any() and first_bad < 0:
            first_bad = q
        ids, rel = ids[valid], rel[valid]
        d = bits[q, rel]
        key = (mono_u32(d.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | (ids & 0xFFFFFFFF).astype(np.uint64)
        order = np.argsort(key, kind="stable")[:k]
        n = len(order)
        dist[q, :n], idx[q, :n], keys[q, :n], count[q] = d[order], ids[order], key[order], n
    return dist, idx, keys, count, first_bad
