"""The scan over the whole dimension range the C ABI promises (include/nlsh_hip.h: 1 <= d <= NLSH_MAX_DIM = 1024), all three schedules
on one deterministic index per dimension, held to the oracle (pinned at the same dimensions by tests/test_oracle_dims_cpu.py).

d4 = ceil(d / 4) is what the kernels' shapes depend on: the pair-unrolled loop and odd-chunk tail of l2_kblock, the chunk clamp of
l2_task's staging when d4 < KBt, the single-stage body's selection (nrows * d4 <= 1024 && nrows <= 64) and its LDS row stride d4 | 1,
the <LPR, VPL> / QB switches of scan_kernel and bscan2_kernel at d4 = 16/17, 32/33, 64/65, 128/129, and the second trip of the 64-wide
loops of gather_rows_kernel and prep_query from d4 > 64 on.  The index is built like tests/test_gpu_tiled_shapes.py builds its own --
injected keys, buckets of chosen sizes probed by chosen numbers of queries, window_rows=0 -- so that the task table the PLAN phase
left proves the shapes ran."""
import numpy as np
import pytest

from helpers import assert_lists_differ_only_at_ties, check_topk_against_candidates, dev, fp64_distances, make_hashing
from helpers import task_table as _task_table
from nlsh_amd import _capi, synth
from oracle import oracle

pytestmark = pytest.mark.gpu

DIMS = [
    1,      # d4 = 1: l2_kblock runs its odd-chunk tail only; one live lane per row in the wave-level kernels
    2,      # d4 = 1, two live elements of the only chunk
    3,      # d4 = 1, the last element before a full chunk
    4,      # d4 = 1 with d % 4 == 0: the tiled scan reads the caller's queries directly, one chunk each
    5,      # d4 = 2: l2_kblock's pair-unrolled loop runs once, no tail
    12,     # d4 = 3 < KBt = 4: the staging clamps chunk indices even in 3- and 4-tile tasks
    13,     # d4 = 4 = KBt of the 3- and 4-tile tasks, < KBt = 8 / 16 of the fatter ones; d % 4 == 1
    16,     # d4 = 4, the same on the direct query path
    17,     # d4 = 5: one chunk past a 4-chunk k-block
    33,     # d4 = 9: one chunk past the 2-tile tasks' 8-chunk k-block
    64,     # d4 = 16: <LPR, VPL> = <16, 1> at its limit; a 64-row task fills the 1024 single-stage slots exactly
    65,     # d4 = 17: first <32, 1> dimension; one chunk past the 1-tile tasks' 16-chunk k-block; single-stage limit 60 rows
    129,    # d4 = 33: first <64, 1> dimension
    256,    # d4 = 64: <64, 1> at its limit, QB = 8 at its limit, the last one-trip dimension of the 64-wide loops
    257,    # d4 = 65: first <64, 2> / QB = 4 dimension; second trip of gather_rows_kernel's and prep_query's loops
    513,    # d4 = 129: first <64, 4> / QB = 2 dimension
    784,    # a real workload width (MNIST)
    960,    # a real workload width (GIST)
    1020,   # d4 = 255: single-stage limit 4 rows, LDS row stride 255
    1021,   # d4 = 256, d % 4 == 1: single-stage limit 4 rows vs 5, LDS row stride 257, three padded elements
    1023,   # d4 = 256, one padded element
    1024,   # NLSH_MAX_DIM: d4 = 256 on the direct query path
]
Q, K = 32, 10
# queries probing a bucket: 1 (three waves hold none), 4 / 5 (one each / one wave holds two), 16 (every wave holds four), 17 (two groups: 16 + 1).
# 11 is there for the waves that hold THREE: queries are dealt round-robin, so a wave holds three only in a group of 9..15 (11: 3, 3, 3, 2),
# which none of the other five counts produces
GROUPS = (1, 4, 5, 11, 16, 17)


def _sizes(d):
    d4 = (d + 3) // 4
    s1 = min(64, 1024 // d4)     # the largest task that takes the single-stage body
    return s1, sorted({1, 2, s1, s1 + 1, 64, 65, 128, 129, 192, 193, 256, 257, 300})


def _build(d, metric, seed):
    """Corpus + per-row bucket keys + per-query key lists: every (bucket size, probing queries) combination once.  Queries 0..29 share
    the buckets at random; query 30 probes nothing and query 31 only the 1- and 2-row buckets (fewer candidates than k)."""
    rng = np.random.default_rng(seed)
    s1, sizes = _sizes(d)
    buckets = [(s, m) for s in sizes for m in GROUPS]
    N = sum(s for s, _ in buckets)
    gen = synth.sift_like if metric == "l2" else synth.glove_like
    corpus, queries = gen(N, d, seed=seed), gen(Q, d, seed=seed + 1)   # integer-valued rows at small d: mass exact ties, intended
    corpus[N // 3:N // 3 + 20] = corpus[:20]                        # exact distance ties across buckets at every d
    bkey = lambda b: int(b * 7 - 200)                               # noqa: E731  signed, gaps between keys
    keys = np.repeat(np.array([bkey(b) for b in range(len(buckets))], np.int32), [s for s, _ in buckets])
    order = rng.permutation(N)                                      # rows of a bucket are scattered over the corpus
    corpus_keys = np.empty(N, np.int32)
    corpus_keys[order] = keys
    key_lists = [[] for _ in range(Q)]
    for b, (s, m) in enumerate(buckets):
        who = [31] if (m == 1 and s <= 2) else rng.choice(Q - 2, size=m, replace=False)
        for q in who:
            key_lists[q].append(bkey(b))
    for q in range(Q):
        rng.shuffle(key_lists[q])
    key_lists[5].insert(2, 999999)                                  # an unknown key in the middle of a list
    assert max(len(ks) for ks in key_lists) <= _capi.MAX_PROBES and not key_lists[30] and len(key_lists[31]) == 2
    return corpus, queries, corpus_keys, key_lists, buckets, s1


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_scan_over_the_dimension_range(metric, d):
    from nlsh_amd.data import Glove, SIFT
    from nlsh_amd.indexer import Indexer
    corpus, queries, corpus_keys, key_lists, buckets, s1 = _build(d, metric, seed=7000 + d)
    d4 = (d + 3) // 4
    Ws, bs = synth.make_weights([d, 8, 16], seed=d)
    hashing = make_hashing(d, (8,), 16, Ws, bs, compat=False)       # the hash is not used: keys are injected on both sides
    cg, qg, kg = dev(corpus), dev(queries), dev(corpus_keys)

    # ---- the references, once: the oracle's lists, and every query's candidate rows with their fp64 distances
    perm, uniq, offs = oracle.build_csr(corpus_keys.astype(np.int64))
    qk, nk = oracle.keys_from_lists(key_lists)
    od, oi, onc = oracle.query_batch(corpus, perm, uniq, offs, queries, qk, nk, K, metric)
    i2r = {int(u): perm[offs[j]:offs[j + 1]] for j, u in enumerate(uniq)}
    cand = []
    for q in range(Q):
        rows = np.concatenate([i2r.get(kk, np.zeros(0, np.int32)) for kk in key_lists[q]] + [np.zeros(0, np.int32)])
        cand.append((rows, fp64_distances(queries[q], corpus[rows], metric)))
    assert int(onc[30]) == 0 and int(onc[31]) == 3 < K              # an empty result and a short one: the padding is exercised

    got = {}
    for algo in ("query", "bucket", "tiled"):
        ix = Indexer(hashing, cg, SIFT.distance if metric == "l2" else Glove.distance, compat=False, algo=algo, corpus_keys=kg, window_rows=0)
        # ---- the index: CSR, the bucket-sorted copy (gather_rows_kernel), its padding columns and the row ids
        assert np.array_equal(ix.perm.cpu().numpy(), perm), algo
        assert ix.row_stride == 4 * d4
        cs = ix.corpus_sorted.cpu().numpy()
        assert np.array_equal(cs[:, :d].view(np.uint32), corpus[perm].view(np.uint32)), algo
        assert not cs[:, d:].view(np.uint32).any(), algo
        assert np.array_equal(ix.gid.cpu().numpy(), perm), algo
        res, nc, dist, idx = ix.query_with_keys(qg, key_lists, k=K)
        assert ix.last_algo == {"query": _capi.SCAN_QUERY_MAJOR, "bucket": _capi.SCAN_BUCKET_MAJOR, "tiled": _capi.SCAN_BUCKET_TILED}[algo]
        assert nc == onc.tolist(), algo
        dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
        got[algo] = (dist, idx)
        if algo == "tiled" and metric == "l2":                      # same k-ascending fmaf chain as the oracle: bit for bit
            assert np.array_equal(idx, oi)
            assert np.array_equal(dist.view(np.uint32), od.view(np.uint32))
        else:
            for q in range(Q):
                n = min(K, int(onc[q]))
                check_topk_against_candidates(idx[q], dist[q], cand[q][0], cand[q][1], K)    # incl. -1 / +inf behind min(k, C_q)
                assert_lists_differ_only_at_ties(idx[q][:n], oi[q][:n], queries[q], corpus, metric)
        if algo != "tiled":
            continue

        # ---- the task table the PLAN phase left proves the shapes ran
        P = max(len(ks) for ks in key_lists)
        nq, nrows = _task_table(ix, Q, P, K, d)
        nq, nrows = nq.tolist(), nrows.tolist()
        assert len(nq) == sum(((m + 15) // 16) * ((s + 255) // 256) for s, m in buckets)
        assert min(nq) == 1 and max(nq) == 16 and min(nrows) >= 1 and max(nrows) <= 256
        assert {(r + 63) // 64 for r in nrows} == {1, 2, 3, 4}
        # queries are dealt round-robin over the 4 waves (NLSH_SLOT): waves holding 0, 1, 2, 3 and 4 queries all occur
        assert {max(0, min(4, (a - wave + 3) // 4)) for a in nq for wave in range(4)} == set(range(5))
        assert s1 in nrows and s1 * d4 <= 1024                      # the single-stage body at its limit
        if s1 < 64:
            assert s1 + 1 in nrows and (s1 + 1) * d4 > 1024         # the fat one-tile body, one row past the limit
        if d4 <= 16:
            # 64 rows x 16 chunks fill the 1024 single-stage slots: every task of <= 64 rows is single-stage, the fat one-tile body
            # cannot occur at these dimensions
            assert not [r for r in nrows if r <= 64 and r * d4 > 1024]

    # the query-major and the wave-level schedule share their arithmetic: bit-identical to each other
    assert np.array_equal(got["query"][1], got["bucket"][1])
    assert np.array_equal(got["query"][0].view(np.uint32), got["bucket"][0].view(np.uint32))


def test_dimension_above_the_limit_is_refused():
    """d = NLSH_MAX_DIM + 1: building an index raises -- with injected keys (the bucket-sorted copy is refused) and without (the encoder
    is refused) -- and nothing is truncated to 1024 columns behind the caller's back."""
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    d = _capi.MAX_DIM + 1
    corpus = synth.sift_like(64, d, seed=1)
    Ws, bs = synth.make_weights([d, 8, 16], seed=1)
    hashing = make_hashing(d, (8,), 16, Ws, bs, compat=False)
    keys = dev(np.arange(64, dtype=np.int32) % 4)
    with pytest.raises(_capi.NlshHipError) as err:
        Indexer(hashing, dev(corpus), SIFT.distance, compat=False, corpus_keys=keys)
    assert str(d) in str(err.value)                                  # refused for its dimension, not for something else
    with pytest.raises(_capi.NlshHipError):
        Indexer(hashing, dev(corpus), SIFT.distance, compat=False)
