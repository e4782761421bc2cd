"""k in 65..256 on the device: the LDS-tiled schedule, its per-query merge, the shard merge and the facade, against the CPU oracle
and against the reference's recorded lists.  Every call below is refused with NLSH_E_UNSUPPORTED by a library whose limit is
k <= 64 everywhere."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import assert_lists_differ_only_at_ties, G, cases, check_topk_against_candidates, dev, make_hashing
from nlsh_amd import synth
from oracle import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "checkpoints", "sift1m_manifold_h16.npz")

WIDE_K = [65, 100, 128, 200, 256]
WIDE_CASES = [
    # metric, d, N, Q, H, P
    ("l2", 128, 20000, 64, 4, 3),        # 16 fat buckets of ~1250 rows: five 256-row segments per probe -> the merge's list table
    ("l2", 128, 20000, 40, 3, 3),        # 8 buckets of ~2500 rows: more than 8 segments per probe -> the merge's shuffle search
    ("l2", 128, 20000, 64, 10, 10),      # many small buckets: most lists shorter than k
    ("cosine", 100, 15000, 50, 6, 6),
    ("cosine", 25, 5000, 33, 5, 4),      # d % 4 != 0
    ("l2", 50, 5000, 33, 5, 4),
    ("cosine", 300, 3000, 20, 4, 3),
    ("l2", 600, 1500, 10, 3, 2),
]


def _oracle_index(ix):
    ck = ix.corpus_keys.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return oracle.build_csr(ck)


def _check_against_oracle(corpus, queries, key_lists, k, metric, nc, dist, idx, perm, uniq, offs, bit_exact):
    Q = len(key_lists)
    qk, nk = oracle.keys_from_lists(key_lists)
    od, oi, onc = oracle.query_batch(corpus, perm, uniq, offs, queries, qk, nk, k, metric)
    assert list(nc) == onc.tolist()                                  # candidate counts: exact
    i2r = {int(u): perm[offs[i]:offs[i + 1]] for i, u in enumerate(uniq)}
    exact = 0
    for q in range(Q):
        rows = [i2r[kk] for kk in dict.fromkeys(key_lists[q]) if kk in i2r]
        rows = np.concatenate(rows) if rows else np.zeros(0, np.int32)
        _, d64 = oracle.distances(queries[q], corpus, rows, metric, f64=True)
        check_topk_against_candidates(idx[q], dist[q], rows, d64, k)
        n = min(k, int(onc[q]))
        exact += int(assert_lists_differ_only_at_ties(idx[q][:n], oi[q][:n], queries[q], corpus, metric))
        assert np.all(idx[q][n:] == -1) and np.all(np.isinf(dist[q][n:]))
    if bit_exact:                                                    # tiled L2: the oracle's k-ascending fmaf chain
        assert exact == Q
        assert np.array_equal(idx, oi)
        assert np.array_equal(dist.view(np.uint32), od.view(np.uint32))
    return onc


@pytest.mark.parametrize("k", WIDE_K)
@pytest.mark.parametrize("metric,d,N,Q,H,P", WIDE_CASES)
def test_wide_k_scan_vs_oracle_shapes(metric, d, N, Q, H, P, k):
    from nlsh_amd.data import Glove, SIFT
    from nlsh_amd.indexer import Indexer
    rng = np.random.default_rng(d * 7 + N + H)
    gen = synth.sift_like if metric == "l2" else synth.glove_like
    corpus, queries = gen(N, d, seed=d), gen(Q, d, seed=d + 1)
    corpus[N // 2:N // 2 + 25] = corpus[:25]                          # exact distance ties
    Ws, bs = synth.make_weights([d, 64, H], seed=d)
    hashing = make_hashing(d, (64,), H, Ws, bs, compat=False)
    indexer = Indexer(hashing, dev(corpus), SIFT.distance if metric == "l2" else Glove.distance, compat=False, algo="tiled")
    perm, uniq, offs = _oracle_index(indexer)
    assert np.array_equal(indexer.perm.cpu().numpy(), perm)
    present = uniq.tolist()
    key_lists = []
    for q in range(Q):
        ks = [int(present[i]) for i in rng.choice(len(present), size=min(P, len(present)), replace=False)]
        if q % 7 == 0:
            ks = ks[:1] + [4000000000 + q] + ks[1:]                  # unknown key in the middle (full-width)
        if q % 11 == 5:
            ks = [4000000000 + q]                                    # C_q = 0
        key_lists.append(ks)
    res, nc, dist, idx = indexer.query_with_keys(dev(queries), key_lists, k=k)
    onc = _check_against_oracle(corpus, queries, key_lists, k, metric, nc, dist.cpu().numpy(), idx.cpu().numpy(), perm, uniq, offs,
                                bit_exact=metric == "l2")
    assert int(onc.min()) == 0 and (int(onc.max()) > k or H == 10)    # (H = 10: ~20-row buckets, the lists are the short ones)
    if H == 3 and N == 20000:                                        # the case that leaves the merge's list table
        assert int(np.diff(offs).max()) > 2048
    for q in range(Q):                                               # the reference-typed lists: min(k, C_q) ids, F7 below k
        assert len(res[q]) == min(k, int(onc[q])) or int(onc[q]) < k


@pytest.mark.parametrize("k", WIDE_K)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_wide_k_candidate_count_edges(metric, k):
    """Buckets of chosen sizes (injected corpus keys): C_q = 0, 0 < C_q < k, C_q == k from one list and from two, k + 1, a bucket of
    several segments, and all of them together."""
    from nlsh_amd.data import Glove, SIFT
    from nlsh_amd.indexer import Indexer
    d, H = 64, 8
    sizes = {1: k, 2: k - 1, 3: 1, 4: k + 1, 5: 700, 6: 3, 7: 256, 8: 257}
    N = sum(sizes.values())
    gen = synth.sift_like if metric == "l2" else synth.glove_like
    corpus, queries = gen(N, d, seed=k), gen(12, d, seed=k + 1)
    ck = np.concatenate([np.full(n, key, np.int32) for key, n in sizes.items()])
    ck = ck[np.random.default_rng(k).permutation(N)]
    corpus[np.nonzero(ck == 5)[0][:20]] = corpus[np.nonzero(ck == 1)[0][:20]]     # exact ties across buckets
    Ws, bs = synth.make_weights([d, 64, H], seed=3)
    hashing = make_hashing(d, (64,), H, Ws, bs, compat=False)
    indexer = Indexer(hashing, dev(corpus), SIFT.distance if metric == "l2" else Glove.distance, compat=False, algo="tiled",
                      corpus_keys=dev(ck))
    perm, uniq, offs = _oracle_index(indexer)
    key_lists = [[99], [], [1], [2], [2, 3], [3, 2], [4], [5], [6, 3], [7], [8], [1, 2, 3, 4, 5, 6, 7, 8]]
    res, nc, dist, idx = indexer.query_with_keys(dev(queries), key_lists, k=k)
    assert nc == [0, 0, k, k - 1, k, k, k + 1, 700, 4, 256, 257, N]
    _check_against_oracle(corpus, queries, key_lists, k, metric, nc, dist.cpu().numpy(), idx.cpu().numpy(), perm, uniq, offs,
                          bit_exact=metric == "l2")


def _small_bucket_setup(N=20000, Q=200, d=128, H=10, seed=31):
    corpus, mean, std = synth.standardise(synth.sift_like(N, d, seed=seed))
    queries, _, _ = synth.standardise(synth.sift_like(Q, d, seed=seed + 1), mean, std)
    Ws, bs = synth.make_weights([d, 64, H], seed=seed)
    return corpus, queries, Ws, bs, make_hashing(d, (64,), H, Ws, bs, compat=False)


def test_wide_k_results_do_not_depend_on_the_window():
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    corpus, queries, Ws, bs, hashing = _small_bucket_setup()
    cd, qd = dev(corpus), dev(queries)
    outs = []
    for w in (0, 64, 128, 256):
        ix = Indexer(hashing, cd, SIFT.distance, compat=False, algo="tiled", window_rows=w)
        keys, nkeys = ix.hash_device(qd, hash_times=10, seed=9)
        outs.append(tuple(t.clone() for t in ix.scan_tensors(qd, keys, nkeys, k=100, want_keys=True)))
        assert ix.last_window == w
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)
    assert int(outs[0][2].max()) > 100 and int((outs[0][1] >= 0).sum()) > 0


def test_wide_k_default_indexer_and_refusals():
    from nlsh_amd import _capi
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    corpus, queries, Ws, bs, hashing = _small_bucket_setup()
    cd, qd = dev(corpus), dev(queries)
    default, tiled = Indexer(hashing, cd, SIFT.distance, compat=False), Indexer(hashing, cd, SIFT.distance, compat=False, algo="tiled")
    a = default.query_tensors(qd, k=100, hash_times=10, seed=4, want_keys=True)          # 2000 pairs: the tiled schedule by default
    assert default.last_algo == _capi.SCAN_BUCKET_TILED
    b = tiled.query_tensors(qd, k=100, hash_times=10, seed=4, want_keys=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ids_a, nc_a = default.query(qd, k=100, hash_times=10, seed=4)
    ids_b, nc_b = tiled.query(qd, k=100, hash_times=10, seed=4)
    assert ids_a == ids_b and nc_a == nc_b

    def refused(fn):
        with pytest.raises(_capi.NlshHipError) as e:
            fn()
        assert e.value.code == _capi.E_UNSUPPORTED
        assert 'algo="tiled"' in str(e.value) and "NLSH_SCAN_BUCKET_TILED" in str(e.value) and "256" in str(e.value)
    k1 = torch.zeros((4, 1), dtype=torch.int32, device="cuda")
    n1 = torch.ones((4,), dtype=torch.int32, device="cuda")
    refused(lambda: default.scan_tensors(qd[:4], k1, n1, k=100))                         # 4 pairs: the query-major stream, k <= 64
    refused(lambda: default.query(qd[:4], k=100, hash_times=1))
    d4 = tiled.scan_tensors(qd[:4], k1, n1, k=100)                                       # the same batch, schedule named: served
    assert d4[0].shape == (4, 100)
    for algo in ("query", "bucket"):
        ix = Indexer(hashing, cd, SIFT.distance, compat=False, algo=algo)
        refused(lambda: ix.query_tensors(qd, k=65, hash_times=10, seed=4))
        refused(lambda: ix.query_tensors(qd[:4], k=256, hash_times=1, seed=4))
    refused(lambda: tiled.query_tensors(qd, k=257, hash_times=10, seed=4))
    # a refusal leaves the index usable
    again = tiled.query_tensors(qd, k=100, hash_times=10, seed=4, want_keys=True)
    for x, y in zip(again, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["l2_k100", "cos_k200"])
def test_g9_query_widek_on_the_device(name):
    """The reference's Indexer.query at k = 100 / 200 on its recorded corpus keys (as test_scan_golden_injected_keys at k = 10)."""
    from nlsh_amd.data import Glove, SIFT
    from nlsh_amd.indexer import Indexer
    meta = json.load(open(os.path.join(G, "g9_query_widek.json")))[name]
    g = np.load(os.path.join(G, "g9_query_widek.npz"))
    corpus, queries, Ws, bs = cases.g5_inputs(meta)
    cos = meta["metric"] == "cosine"
    hashing = make_hashing(meta["d"], (64, 64), meta["H"], Ws, bs, tanh=cos)
    indexer = Indexer(hashing, dev(corpus), Glove.distance if cos else SIFT.distance, algo="tiled",
                      corpus_keys=dev(g[name + "/corpus_keys"].astype(np.int32)))
    res, nc, dist, idx = indexer.query_with_keys(dev(queries), meta["injected_iter"], k=meta["k"])
    assert nc == g[name + "/ncand"].tolist()
    off = g[name + "/cand_off"]
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    full = 0
    for q in range(meta["Q"]):
        rows = g[name + "/cand_rows"][off[q]:off[q + 1]]
        dref = g[name + "/cand_dist"][off[q]:off[q + 1]]
        ref_ids = meta["result_ids"][q]
        if nc[q] < meta["k"]:
            assert res[q] == ref_ids                               # F7 fallback list: exact
        else:
            full += 1
            cases.assert_topk_equivalent(res[q], ref_ids, rows, dref, meta["k"], 1e-4)
        _, d64 = oracle.distances(queries[q], corpus, rows, meta["metric"], f64=True)
        check_topk_against_candidates(idx[q], dist[q], rows, d64, meta["k"])
    assert full >= 9
    rec = oracle.calculate_recall(list(g[name + "/ground_truth"]), res)
    swapped = sum(len(set(res[q]) - set(meta["result_ids"][q])) for q in range(meta["Q"]))
    assert abs(np.mean(rec) - meta["mean_recall"]) <= swapped / (meta["k"] * meta["Q"]) + 1e-12


def test_wide_k_one_call_equals_separate_calls_and_pipeline_slots():
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.pipeline import QueryPipeline
    k, P = 100, 10
    corpus, queries, Ws, bs, hashing = _small_bucket_setup(N=60000, Q=2000, H=9, seed=41)
    ix = Indexer(hashing, dev(corpus), SIFT.distance)
    batches = [torch.roll(dev(queries), shifts=13 * i, dims=0).contiguous() for i in range(4)]
    want = []
    for i, b in enumerate(batches):
        keys, nkeys = ix.hash_device(b, hash_times=P, seed=70 + i)
        sep = ix.scan_tensors(b, keys, nkeys, k=k)[:3]
        one = ix.query_tensors(b, k=k, hash_times=P, seed=70 + i)[:3]                      # the fused nlsh_query_batch path
        for x, y in zip(sep, one):
            assert torch.equal(x, y)
        want.append(tuple(t.clone() for t in one))
    assert int(want[0][2].max()) > k
    for graph in (False, True):
        pipe = QueryPipeline(ix, batches[0], k=k, hash_times=P, depth=2, graph=graph)
        assert pipe.graph == graph
        for i, b in enumerate(batches):
            out = pipe.submit(b, seed=70 + i)
            pipe.synchronize()
            for x, y in zip(out[:3], want[i]):
                assert torch.equal(x, y), (graph, i)
        assert not pipe.overflowed()
        pipe.close()
    # the task table far too small: the checked call grows it and converges on the same answer
    tkey = ix._last_tkey
    ix._max_tasks[tkey] = 5
    again = ix.query_tensors(batches[0], k=k, hash_times=P, seed=70)[:3]
    assert ix._max_tasks[tkey] > 5
    for x, y in zip(again, want[0]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("k", [100, 256])
def test_wide_k_sharded_scan_plus_merge_equals_single_index(k):
    from nlsh_amd.data import SIFT
    from nlsh_amd.distributed import merge_topk_device, shard_range
    from nlsh_amd.indexer import Indexer
    N, Q, d, H, P, n_shards = 30000, 200, 128, 5, 6, 8
    corpus, _, _ = synth.standardise(synth.sift_like(N, d, seed=8))
    queries, _, _ = synth.standardise(synth.sift_like(Q, d, seed=9))
    corpus[100:140] = corpus[20000:20040]                          # exact ties across shards
    Ws, bs = synth.make_weights([d, 64, H], seed=8)
    hashing = make_hashing(d, (64,), H, Ws, bs)
    qd, cd = dev(queries), dev(corpus)
    single = Indexer(hashing, cd, SIFT.distance)
    d1, i1, n1, _ = single.query_tensors(qd, k=k, hash_times=P, seed=77)
    assert int(n1.max()) > k                                        # (a shard's own lists are mostly short ones at these sizes)
    keys_all, nc_all = [], []
    for r in range(n_shards):
        lo, hi = shard_range(N, r, n_shards)
        sh = Indexer(hashing, cd[lo:hi], SIFT.distance, id_base=lo)
        _, _, nc, k64 = sh.query_tensors(qd, k=k, hash_times=P, seed=77, want_keys=True)
        keys_all.append(k64); nc_all.append(nc)
    packed = torch.cat([torch.stack(keys_all), torch.stack(nc_all).long()[:, :, None]], dim=2)
    dm, im, nm = merge_topk_device(packed, k)
    assert torch.equal(nm, n1) and torch.equal(im, i1) and torch.equal(dm, d1)


def test_wide_k_sliced_scan_hash_times_100():
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    d, H, N, Q, k, P = 128, 14, 30000, 96, 100, 100
    Ws, bs = synth.make_weights([d, 64, H], seed=77)
    corpus, _, _ = synth.standardise(synth.sift_like(N, d, seed=70))
    queries, _, _ = synth.standardise(synth.sift_like(Q, d, seed=71))
    hashing = make_hashing(d, (64,), H, Ws, bs, compat=False)
    qd = dev(queries)
    keys, nkeys = hashing.hash_device(qd, n=P, seed=5)
    assert int(nkeys.max()) > 64                                    # more than one slice
    indexer = Indexer(hashing, dev(corpus), SIFT.distance, compat=False)
    dist, idx, nc, _ = indexer.scan_tensors(qd, keys, nkeys, k=k)
    perm, uniq, offs = _oracle_index(indexer)
    od, oi, onc = oracle.query_batch(corpus, perm, uniq, offs, queries, keys.cpu().numpy().astype(np.int64) & 0xFFFFFFFF,
                                     nkeys.cpu().numpy(), k, "l2")
    assert np.array_equal(nc.cpu().numpy(), onc) and int(onc.max()) > k
    assert np.array_equal(idx.cpu().numpy(), oi)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), od.view(np.uint32))


@pytest.mark.parametrize("k", [100, 130, 256])
def test_merge_topk_with_repeated_lists_stays_inside_its_rows(k):
    """nlsh_merge_topk takes whatever lists a C caller hands it: the same list five times over (every key repeated, so the tie search
    can select more than k; which copies survive the cut is not defined) must fill each query's k slots, in order, with keys it was
    given, starting at the smallest, and write nothing behind them."""
    from nlsh_amd import _capi
    Q, n_lists, pad = 7, 5, 64
    rng = np.random.default_rng(k)
    dists = np.sort(rng.random((Q, k)).astype(np.float32), axis=1)
    dists[:, 10:14] = dists[:, 10:11]                               # equal distances inside a list as well
    ids = rng.permutation(Q * k).reshape(Q, k).astype(np.int64)
    mono = dists.view(np.uint32).astype(np.int64) | (1 << 31)       # positive floats: bits with the sign set
    keys = (mono << 32) | ids
    keys[3, k // 2:] = -1                                           # a short list (~0 padded)
    keys = np.sort(keys.view(np.uint64), axis=1).view(np.int64)
    packed = dev(np.broadcast_to(keys[None], (n_lists, Q, k)).copy())
    out_dist = torch.full((Q * k + pad,), -7.0, dtype=torch.float32, device="cuda")
    out_idx = torch.full((Q * k + pad,), -7, dtype=torch.int32, device="cuda")
    _capi.check(_capi.lib().nlsh_merge_topk(packed.data_ptr(), k, n_lists, Q, k, None, out_dist.data_ptr(), out_idx.data_ptr(), None,
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((out_dist[Q * k:] == -7.0).all()) and bool((out_idx[Q * k:] == -7).all())
    gd, gi = out_dist[:Q * k].view(Q, k).cpu().numpy(), out_idx[:Q * k].view(Q, k).cpu().numpy()
    assert not (gd == -7.0).any() and not (gi == -7).any()          # every slot written
    for q in range(Q):
        real = keys[q][keys[q] != -1]
        given = set((real & 0xFFFFFFFF).tolist()) | {-1}
        assert set(gi[q].tolist()) <= given, q
        assert gi[q][0] == int(real[0] & 0xFFFFFFFF) and gd[q][0] == dists[q][0]
        assert np.all(np.diff(gd[q]) >= 0)
        n_real = int((gi[q] >= 0).sum())
        assert n_real == min(k, n_lists * len(real)) and np.all(gi[q][n_real:] == -1) and np.all(np.isinf(gd[q][n_real:]))


# ----------------------------------------------------------------------------- full size (BASELINE.json configs[1])
@pytest.fixture(scope="module")
def sift1m():
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    N, Q, d = 1_000_000, 10_000, 128
    corpus, mean, std = synth.standardise(synth.sift_manifold(N, d, seed=synth.SEED_DATA))
    queries, _, _ = synth.standardise(synth.sift_manifold(Q, d, seed=synth.SEED_QUERY), mean, std)
    arrs = np.load(CKPT)
    Ws, bs = [arrs[f"W{i}"] for i in range(3)], [arrs[f"b{i}"] for i in range(3)]
    hashing = make_hashing(d, (256, 256), 16, Ws, bs)
    cg, qg = dev(corpus), dev(queries)
    return dict(corpus=corpus, queries=queries, cg=cg, qg=qg, ix=Indexer(hashing, cg, SIFT.distance, algo="tiled"))


def test_wide_k_full_size_all_queries_vs_oracle(sift1m, capsys):
    """1M x 128, 10^4 queries, 16-bit hash, 10 probes, k = 100: every query against the oracle (counts, ids, distance bits), the
    reference-typed lists against the oracle's F7 rule, and recall@100 printed (a figure to record, not a gate)."""
    from nlsh_amd.data import brute_force_topk
    from nlsh_amd.metrics import calculate_recall
    ix, qg, k, P, seed = sift1m["ix"], sift1m["qg"], 100, 10, 5000
    Q = qg.shape[0]
    keys, nkeys = ix.hash_device(qg, hash_times=P, seed=seed)
    dist, idx, nc, _ = ix.scan_tensors(qg, keys, nkeys, k=k)
    kh, nh = keys.cpu().numpy().astype(np.int64), nkeys.cpu().numpy()
    ox = oracle.OracleIndexer.from_keys(sift1m["corpus"], ix.corpus_keys.cpu().numpy())
    od, oi, onc = oracle.query_batch(ox.corpus, ox.perm, ox.uniq_keys, ox.offsets, sift1m["queries"], kh, nh, k, "l2", simd=True)
    assert np.array_equal(nc.cpu().numpy(), onc)
    assert np.array_equal(idx.cpu().numpy(), oi)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), od.view(np.uint32))
    ids, ncand = ix.query(qg, k=k, hash_times=P, seed=seed)
    key_lists = [list(set(int(v) for v in kh[i, :nh[i]])) for i in range(Q)]
    ores, oncl, _, _ = ox.query_with_keys(sift1m["queries"], key_lists, k, simd=True)
    assert ncand == oncl
    assert ids == ores
    short = sum(1 for c in oncl if c < k)
    assert short > 0
    gt = brute_force_topk(qg, sift1m["cg"], k, "l2").cpu().numpy()
    rec = calculate_recall(list(gt), ids, np.mean)
    with capsys.disabled():
        print(f"\n[wide k, SIFT1M] all {Q} queries bit-identical to the oracle at k = {k}; {short} short queries (F7); "
              f"recall@{k} = {rec:.4f} at {np.mean(ncand):.1f} candidates per query")
