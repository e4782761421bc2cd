"""Exact re-ranking against ITS DEFINITION: the re-rank of a query is the k smallest (distance bits, id) keys over the
valid ids of its candidate list, the distance of a pair having the bits the tiled float32 scan gives that pair.  The reference is
tests/refine_ref.py -- float32 twin indexes over the original rows (one bucket of at most 256 rows each, scanned with k = rows), for L2
also the oracle, and a numpy selection -- never the code under test.  Every comparison is on raw bits: no tolerance anywhere."""
import numpy as np
import pytest
import torch

from helpers import dev, make_hashing
from nlsh_amd import _capi, synth
from refine_ref import pair_bits, rerank_reference

pytestmark = pytest.mark.gpu

GUARD = 64                      # words behind every output that must keep their sentinel
METRIC_CODE = {"l2": _capi.METRIC_L2_EPS, "cosine": _capi.METRIC_COSINE}


def _dist(metric):
    from nlsh_amd.data import Glove, SIFT
    return SIFT.distance if metric == "l2" else Glove.distance


def _hasher(d, H=16, seed=None, compat=False, mean=0.0, spread=1.0):
    Ws, bs = synth.make_weights([d, 8, H], seed=d if seed is None else seed)
    Ws[0] = (Ws[0] / spread).astype(np.float32)
    bs[0] = (bs[0] - Ws[0].sum(1) * mean).astype(np.float32)
    return make_hashing(d, (8,), H, Ws, bs, compat=compat)


def _store(rows, metric, **kw):
    from nlsh_amd.refine import RefineStore
    return RefineStore(rows if isinstance(rows, torch.Tensor) else dev(rows), metric, **kw)


def call_rerank(store, queries, cand, kc, k, id_base=None, on_host=None, want_keys=True, want_count=True):
    """`nlsh_rerank_topk` as a pure function on buffers of this test's own, each with GUARD sentinel words behind it ->
    (dist, idx, keys uint64 | None, count | None, first_bad) as numpy; asserts that nothing was written behind an output."""
    Q = int(queries.shape[0])
    od = torch.full((Q * k + GUARD,), -7.5, dtype=torch.float32, device="cuda")
    oi = torch.full((Q * k + GUARD,), -77, dtype=torch.int32, device="cuda")
    ok = torch.full((Q * k + GUARD,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    oc = torch.full((Q + GUARD,), -77, dtype=torch.int32, device="cuda")
    fb = torch.full((1 + GUARD,), -77, dtype=torch.int32, device="cuda")
    rc = _capi.lib().nlsh_rerank_topk(
        queries.data_ptr(), queries.stride(0), Q, queries.shape[1], store.rows.data_ptr(), store.stride, store.n_rows,
        store.id_base if id_base is None else id_base, int(store.where == "host") if on_host is None else on_host,
        _capi.ptr(store.inv_norm), cand.data_ptr(), cand.stride(0), kc, k, METRIC_CODE[store.metric],
        od.data_ptr(), oi.data_ptr(), ok.data_ptr() if want_keys else None, oc.data_ptr() if want_count else None, fb.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    _capi.check(rc)
    od, oi, ok, oc, fb = (t.cpu().numpy() for t in (od, oi, ok, oc, fb))
    assert (od[Q * k:] == np.float32(-7.5)).all() and (oi[Q * k:] == -77).all() and (ok[Q * k:] == 0x5A5A5A5A).all()
    assert (oc[Q:] == -77).all() and (fb[1:] == -77).all()
    if not want_keys:
        assert (ok == 0x5A5A5A5A).all()
    if not want_count:
        assert (oc == -77).all()
    return (od[:Q * k].reshape(Q, k), oi[:Q * k].reshape(Q, k), ok[:Q * k].reshape(Q, k).view(np.uint64) if want_keys else None,
            oc[:Q] if want_count else None, int(fb[0]))


def assert_is_the_reference(got, bits, cand, k, id_base, what, first_bad=-1):
    dist, idx, keys, count, fb = got
    rd, ri, rk, rc, rfb = rerank_reference(bits, cand, k, id_base)
    assert rfb == first_bad and fb == first_bad, (what, fb, rfb)
    assert np.array_equal(idx, ri), what
    assert np.array_equal(dist.view(np.uint32), rd.view(np.uint32)), what
    if keys is not None:
        assert np.array_equal(keys, rk), what
    if count is not None:
        assert np.array_equal(count, rc), what


# ------------------------------------------------------------------------------------------------ 1. the entry point as a pure function
N_PURE, Q_PURE = 600, 5
_worlds = {}


def _world(d, metric):
    """Rows, queries, the pair table (computed once, shared, never changed) and a device store of one (d, metric)."""
    key = (d, metric)
    if key not in _worlds:
        rng = np.random.default_rng(100 * d + (metric == "cosine"))
        rows = (rng.standard_normal((N_PURE, d)) * rng.uniform(0.2, 3.0, size=d)).astype(np.float32)
        queries = (rng.standard_normal((Q_PURE, d)) * 1.5).astype(np.float32)
        bits = pair_bits(rows, queries, metric, _hasher(d))
        bits.setflags(write=False)
        _worlds[key] = dict(rows=rows, queries=queries, bits=bits, store=_store(rows, metric))
    return _worlds[key]


def _lists(rng, Q, kc, id_base, n_rows):
    return np.stack([id_base + rng.choice(n_rows, kc, replace=False) for _ in range(Q)]).astype(np.int32)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("d", [1, 3, 4, 5, 100, 128, 260, 1024])
def test_rerank_equals_the_definition_word_for_word(d, metric):
    """d: pitch padding and non-multiples of 4, one stage and many; kc: either side of one and two 64-candidate groups, the narrow and the
    wide selection; k: 1 .. kc; Q = 5 is one more than a workgroup's four queries (two at d = 1024, kc > 64: also a partial last
    workgroup); ids based at 0, 1000 and below zero."""
    w = _world(d, metric)
    store, bits = w["store"], w["bits"]
    qd = dev(w["queries"])
    rng = np.random.default_rng(d)
    for kc in (1, 63, 64, 65, 128, 129, 256):
        for id_base in (0, 1000, -5000):
            cand = _lists(rng, Q_PURE, kc, id_base, N_PURE)
            if kc >= 3:
                cand[0, kc // 2] = -1           # padding in the middle of a list
            cd = dev(cand)
            for k in sorted({kk for kk in (1, 10, 64, 65, 256, kc) if kk <= kc}):
                for Q in (1, Q_PURE):
                    got = call_rerank(store, qd[:Q], cd[:Q], kc, k, id_base=id_base)
                    assert_is_the_reference(got, bits[:Q], cand[:Q], k, id_base, (d, metric, kc, k, Q, id_base))


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_special_lists_views_and_store_pitch(metric):
    d, kc, k = 100, 40, 10
    w = _world(d, metric)
    bits, rng = w["bits"], np.random.default_rng(3)
    cand = _lists(rng, Q_PURE, kc, 0, N_PURE)
    cand[0, 17] = -1                            # -1 in the middle
    cand[1, :] = -1                             # an all-padding list
    cand[2, 4:] = -1                            # fewer than k valid ids
    cand[3, ::2] = -1
    cd, qd = dev(cand), dev(w["queries"])
    got = call_rerank(w["store"], qd, cd, kc, k)
    assert_is_the_reference(got, bits, cand, k, 0, "special lists")
    assert got[3].tolist() == [10, 0, 4, 10, 10] and (got[1][1] == -1).all() and np.isposinf(got[0][1]).all()
    # optional outputs stay untouched when they are not asked for
    assert_is_the_reference(call_rerank(w["store"], qd, cd, kc, k, want_keys=False, want_count=False), bits, cand, k, 0, "no keys, no counts")
    # strided and misaligned query views; a candidate table that is a column range of a wider one
    wide_q = torch.zeros((Q_PURE, d + 11), dtype=torch.float32, device="cuda")
    wide_q[:, 1:d + 1] = qd
    wide_c = torch.full((Q_PURE, kc + 9), 123456789, dtype=torch.int32, device="cuda")
    wide_c[:, 3:kc + 3] = cd
    assert_is_the_reference(call_rerank(w["store"], wide_q[:, 1:d + 1], wide_c[:, 3:kc + 3], kc, k), bits, cand, k, 0, "views")
    # a prefix of every list: kc below the table's width
    assert_is_the_reference(call_rerank(w["store"], qd, cd, 7, 7), bits, cand[:, :7], 7, 0, "prefix")
    # row_align=32: every row on a 128-byte line, same bits
    padded = _store(w["rows"], metric, row_align=32)
    assert padded.stride == 128 and w["store"].stride == 100
    assert_is_the_reference(call_rerank(padded, qd, cd, kc, k), bits, cand, k, 0, "row_align=32")
    # the facade on the same lists
    fd, fi, fc, fk = w["store"].rerank(qd, cd, k, want_keys=True)
    assert_is_the_reference((fd.cpu().numpy(), fi.cpu().numpy(), fk.cpu().numpy().view(np.uint64), fc.cpu().numpy(), -1), bits, cand, k, 0, "facade")


# ------------------------------------------------------------------------------------------------ 2. hard values
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_mass_ties_and_a_query_that_is_a_row(metric):
    rng = np.random.default_rng(8)
    d, N, Q, kc = 20, 300, 6, 256
    base = rng.standard_normal((8, d)).astype(np.float32)
    rows = base[rng.integers(0, 8, size=N)]                     # eight distinct rows: every distance is shared by ~37 ids
    queries = rng.standard_normal((Q, d)).astype(np.float32)
    queries[:3] = rows[[5, 77, 201]]                            # queries that ARE corpus rows
    bits = pair_bits(rows, queries, metric, _hasher(d))
    cand = _lists(rng, Q, kc, 0, N)
    store = _store(rows, metric)
    for k in (1, 10, 64, 100, 256):
        got = call_rerank(store, dev(queries), dev(cand), kc, k)
        assert_is_the_reference(got, bits, cand, k, 0, (metric, k))
    d10, i10 = got[0][:, :40], got[1][:, :40]
    tie = d10[:, 1:] == d10[:, :-1]
    assert tie.sum() > 100 and (i10[:, 1:][tie] > i10[:, :-1][tie]).all(), "equal distances come in id order"


@pytest.mark.parametrize("scale", [1e-25, 3e-16, 1e-12, 1.0, 3e18])
def test_l2_at_extreme_magnitudes(scale):
    """Both sides of the epilogue's 2^-96 guard, the zero distance of a query that is a row, sums that underflow and sums that overflow:
    the cases and shapes of test_tiled_l2_at_extreme_magnitudes_is_still_the_oracle_bit_for_bit."""
    rng = np.random.default_rng(11)
    d, k, N, Qn, kc = 64, 10, 3000, 48, 256
    rows = (rng.standard_normal((N, d)) * scale).astype(np.float32)
    queries = (rng.standard_normal((Qn, d)) * scale).astype(np.float32)
    twins = rng.choice(N, 16, replace=False)
    queries[:16] = rows[twins]
    bits = pair_bits(rows, queries, "l2", _hasher(d))
    cand = _lists(rng, Qn, kc, 0, N)
    for i, row in enumerate(twins):
        if row not in cand[i]:
            cand[i, 100] = row
    got = call_rerank(_store(rows, "l2"), dev(queries), dev(cand), kc, k)
    assert_is_the_reference(got, bits, cand, k, 0, scale)
    if scale == 1.0:
        assert np.array_equal(got[1][:16, 0], twins) and (got[0][:16, 0] < 1e-4).all()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_non_finite_rows_are_ordered_as_the_scan_orders_them(metric):
    rng = np.random.default_rng(9)
    d, N, Q, kc = 12, 300, 5, 128
    rows = rng.standard_normal((N, d)).astype(np.float32)
    rows[rng.choice(N, 30, replace=False), rng.integers(0, d, 30)] = np.nan
    rows[rng.choice(N, 30, replace=False), rng.integers(0, d, 30)] = np.inf
    rows[rng.choice(N, 30, replace=False), rng.integers(0, d, 30)] = -np.inf
    rows[7] = 0.0                                               # a zero row: cosine's norm floor
    queries = rng.standard_normal((Q, d)).astype(np.float32)
    bits = pair_bits(rows, queries, metric, _hasher(d), check_oracle=False)
    assert np.isnan(bits).any()
    cand = _lists(rng, Q, kc, 0, N)
    store = _store(rows, metric)
    for k in (10, 128):
        assert_is_the_reference(call_rerank(store, dev(queries), dev(cand), kc, k), bits, cand, k, 0, (metric, k))


# ------------------------------------------------------------------------------------------------ 3. ids outside the store
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_ids_outside_the_store_are_dropped_and_reported(metric):
    """Not a fault test: an id outside [id_base, id_base + n_rows) forms no address, by construction of the kernel."""
    d, kc, k, id_base = 100, 70, 10, 1000
    w = _world(d, metric)
    rng = np.random.default_rng(4)
    clean = _lists(rng, Q_PURE, kc, id_base, N_PURE)
    cand = clean.copy()
    cand[3, 0] = id_base + N_PURE               # one past the store
    cand[3, 69] = id_base - 1                   # just below it
    cand[1, 33] = id_base - 10 ** 9             # far below id_base
    cand[4, 64] = -(1 << 31)                    # INT32_MIN
    store = _store(w["rows"], metric, id_base=id_base)
    got = call_rerank(store, dev(w["queries"]), dev(cand), kc, k)
    assert_is_the_reference(got, w["bits"], cand, k, id_base, "bad ids", first_bad=1)
    # every other query's output is what the clean table gives
    ref = call_rerank(store, dev(w["queries"]), dev(clean), kc, k)
    assert ref[4] == -1
    for q in (0, 2):
        assert np.array_equal(got[1][q], ref[1][q]) and np.array_equal(got[2][q], ref[2][q])
    # an empty store: every id is outside it
    empty = _store(w["rows"][:0], metric, id_base=id_base)
    d0, i0, c0 = (_np(t) for t in empty.rerank(dev(w["queries"]), dev(clean), k, check=False))
    assert int(empty.last_first_bad.item()) == 0 and (i0 == -1).all() and np.isposinf(d0).all() and (c0 == 0).all()
    # the facade raises, naming the query
    with pytest.raises(ValueError, match="query 1"):
        store.rerank(dev(w["queries"]), dev(cand), k)
    with pytest.raises(ValueError, match="-1"):
        _store(w["rows"], metric, id_base=-5)    # the row with id -1 cannot be told from padding


# ------------------------------------------------------------------------------------------------ 4. the facade on every storage
D_F, N_F, Q_F, H_F = 24, 2500, 24, 6
_facade = {}


def _facade_world(storage, metric):
    """Rows the storage holds (uint8: integers; the others: real values, which float16 and sq8 round), queries near them, one hasher and
    the pair table over the ORIGINAL rows; computed once per (value kind, metric)."""
    kind = "int" if storage == "uint8" else "real"
    if (kind, metric) not in _facade:
        rng = np.random.default_rng(40 + (kind == "int"))
        if kind == "int":
            rows = rng.integers(0, 256, size=(N_F, D_F)).astype(np.float32)
            queries = (rows[rng.integers(0, N_F, Q_F)] + rng.integers(-20, 21, size=(Q_F, D_F))).astype(np.float32)
            mean, spread = 127.5, 74.0
        else:
            rows = (rng.standard_normal((N_F, D_F)) * rng.uniform(0.5, 2.0, size=D_F)).astype(np.float32)
            queries = (rows[rng.integers(0, N_F, Q_F)] + 0.3 * rng.standard_normal((Q_F, D_F))).astype(np.float32)
            mean, spread = 0.0, 1.0
        hashing = _hasher(D_F, H=H_F, seed=77, mean=mean, spread=spread)
        bits = pair_bits(rows, queries, metric, hashing)
        bits.setflags(write=False)
        _facade[(kind, metric)] = dict(rows=rows, queries=queries, bits=bits, mean=mean, spread=spread)
    return _facade[(kind, metric)]


def _np(t):
    return t.cpu().numpy()


def assert_refined(ix, q, bits, k, what, refine_k=None, **kw):
    """`query_tensors` with the stage on == the definition applied to the same index's own stage-one lists at k1."""
    k1 = refine_k or min(256, 4 * k)
    _, i1, nc1, _ = ix.query_tensors(q, k=k1, refine_k=0, **kw)
    assert not ix.last_query_path.endswith("+refine")
    dist, idx, nc, keys = ix.query_tensors(q, k=k, want_keys=True, refine_k=refine_k, **kw)
    assert ix.last_query_path.endswith("+refine"), what
    rd, ri, rk, _, fb = rerank_reference(bits, _np(i1), k, ix.id_base)
    assert fb == -1
    assert np.array_equal(_np(idx), ri), what
    assert np.array_equal(_np(dist).view(np.uint32), rd.view(np.uint32)), what
    assert np.array_equal(_np(keys).view(np.uint64), rk), what
    assert torch.equal(nc, nc1), what                   # n_candidates is stage one's
    return _np(i1), ri


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("storage", ["sq8", "float16", "uint8", "float32"])
def test_refined_query_tensors_equals_the_definition_on_its_own_stage_one_lists(storage, metric):
    from nlsh_amd.indexer import Indexer
    w = _facade_world(storage, metric)
    hashing = _hasher(D_F, H=H_F, seed=77, mean=w["mean"], spread=w["spread"])
    ix = Indexer(hashing, dev(w["rows"]), _dist(metric), compat=False, storage=storage, refine="device")
    assert ix.refine_store.n_rows == N_F and ix.refine_store.where == "device"
    q = dev(w["queries"])
    deny = ix.row_filter(deny=list(range(0, N_F, 3)))
    variants = [("sampled", dict(hash_times=10, seed=3)), ("ranked", dict(hash_times=10, probes="ranked")),
                ("budget", dict(hash_times=16, probes="ranked", candidate_budget=300)), ("filter", dict(hash_times=10, seed=3, filter=deny))]
    changed = 0
    for name, kw in variants:
        for k in (1, 10, 64):
            i1, ri = assert_refined(ix, q, w["bits"], k, (storage, metric, name, k), **kw)
            changed += int((ri != i1[:, :k]).any())
        if name == "filter":
            assert (ri[ri >= 0] % 3 != 0).all()
    assert_refined(ix, q, w["bits"], 10, "refine_k=256", refine_k=256, hash_times=10, seed=3)
    assert_refined(ix, q, w["bits"], 10, "refine_k=k", refine_k=10, hash_times=10, seed=3)
    # refine_k=0 is the index without the stage; scan_tensors refines as query_tensors does
    keys, nkeys = ix.hash_device(q, hash_times=10, seed=3)
    plain = ix.scan_tensors(q, keys, nkeys, k=40, refine_k=0)
    got = ix.scan_tensors(q, keys, nkeys, k=10, want_keys=True)
    rd, ri, rk, _, _ = rerank_reference(w["bits"], _np(plain[1]), 10, 0)
    assert np.array_equal(_np(got[1]), ri) and np.array_equal(_np(got[0]).view(np.uint32), rd.view(np.uint32))
    assert np.array_equal(_np(got[3]).view(np.uint64), rk)
    if storage in ("sq8", "float16"):
        assert changed, "a lossy storage whose stage-one order is never corrected tests nothing"


@pytest.mark.parametrize("storage", ["sq8", "float32"])
def test_query_lists_with_the_short_query_rule(storage):
    """`query()`: the refined ids where a query has k candidates, the reference's F7 rule -- from stage one's counts -- where it has not."""
    from nlsh_amd.indexer import Indexer
    w = _facade_world(storage, "l2")
    hashing = _hasher(D_F, H=H_F, seed=77, compat=True)
    ix = Indexer(hashing, dev(w["rows"]), _dist("l2"), compat=True, storage=storage, refine="device")
    q = dev(w["queries"])
    short = full = 0
    for k, kw in ((10, dict(hash_times=10, seed=5)), (64, dict(hash_times=10, seed=5)), (200, dict(hash_times=3, seed=5))):
        lists, counts = ix.query(q, k=k, **kw)
        assert ix.last_query_path.endswith("+refine")
        plain, plain_counts = ix.query(q, k=k, refine_k=0, **kw)
        _, idx, nc, _ = ix.query_tensors(q, k=k, **kw)
        idx, nc = _np(idx), _np(nc)
        assert counts == plain_counts == nc.tolist()
        for qi in range(Q_F):
            if nc[qi] < k:
                assert lists[qi] == plain[qi], (k, qi)      # F7: the rows of the last key, as on the unrefined index
                short += 1
            else:
                assert lists[qi] == idx[qi].tolist(), (k, qi)
                full += 1
    assert short and full


# ------------------------------------------------------------------------------------------------ 5. identity, 6. folded
def test_a_float32_exact_index_returns_the_head_of_its_own_list():
    from nlsh_amd.indexer import Indexer
    w = _facade_world("float32", "l2")
    ix = Indexer(_hasher(D_F, H=H_F, seed=77), dev(w["rows"]), _dist("l2"), compat=False, refine="device")
    q = dev(w["queries"])
    for k in (1, 10, 64):
        d1, i1, _, _ = ix.query_tensors(q, k=min(256, 4 * k), hash_times=10, seed=3, refine_k=0)
        dist, idx, _, _ = ix.query_tensors(q, k=k, hash_times=10, seed=3)
        assert torch.equal(idx, i1[:, :k]) and torch.equal(dist.view(torch.int32), d1[:, :k].contiguous().view(torch.int32))


def test_a_folded_index_returns_the_exact_forms_bits():
    from nlsh_amd.indexer import Indexer
    w = _facade_world("float32", "l2")
    hashing = _hasher(D_F, H=H_F, seed=77)
    folded = Indexer(hashing, dev(w["rows"]), _dist("l2"), compat=False, algo="tiled", l2_form="folded", refine="device")
    exact = Indexer(hashing, dev(w["rows"]), _dist("l2"), compat=False, algo="tiled", corpus_keys=folded.corpus_keys)
    q = dev(w["queries"])
    keys, nkeys = folded.hash_device(q, hash_times=10, seed=3)
    dist, idx, _, _ = folded.scan_tensors(q, keys, nkeys, k=10)
    idx_h, dist_h = _np(idx), _np(dist)
    for qi in range(Q_F):
        for j in range(10):
            if idx_h[qi, j] >= 0:
                assert dist_h[qi, j].view(np.uint32) == w["bits"][qi, idx_h[qi, j]].view(np.uint32)
    assert_refined(folded, q, w["bits"], 10, "folded", hash_times=10, seed=3)
    # ... which are the exact-form index's for the same (query, id)
    de, ie, _, _ = exact.scan_tensors(q, keys, nkeys, k=256)
    de, ie = _np(de), _np(ie)
    for qi in range(Q_F):
        of = dict(zip(ie[qi].tolist(), de[qi].view(np.uint32).tolist()))
        for j in range(10):
            if idx_h[qi, j] in of:
                assert of[int(idx_h[qi, j])] == int(dist_h[qi, j].view(np.uint32))
    unrefined = folded.scan_tensors(q, keys, nkeys, k=10, refine_k=0)[0]
    assert not torch.equal(unrefined.view(torch.int32), dist.view(torch.int32)), "the folded form differs somewhere, or the test shows nothing"


# ------------------------------------------------------------------------------------------------ 7. monotone recall, derived
def test_refined_recall_is_never_below_unrefined_recall():
    """F = the float32 index's list, C1 = the sq8 index's stage-one set at k1, both over the same buckets and the same key table.
    refined = top-k of C1 by the exact key and F = top-k of a superset by the same key, so refined & F == C1 & F; the unrefined list is a
    subset of C1, so |refined & F| >= |unrefined & F|.  Both follow from the total (bits, id) order: no threshold."""
    from nlsh_amd.indexer import Indexer
    N, d, Q, k = 3000, 50, 64, 10
    rows = synth.glove_manifold(N, d=d, seed=3)
    queries = synth.glove_manifold(Q, d=d, seed=4)
    hashing = _hasher(d, H=5, seed=9)
    for metric in ("l2", "cosine"):
        sq = Indexer(hashing, dev(rows), _dist(metric), compat=False, storage="sq8", refine="device")
        f32 = Indexer(hashing, dev(rows), _dist(metric), compat=False, algo="tiled", corpus_keys=sq.corpus_keys)
        q = dev(queries)
        keys, nkeys = sq.hash_device(q, hash_times=4, seed=1)
        F = _np(f32.scan_tensors(q, keys, nkeys, k=k)[1])
        gained = 0
        for factor_k1 in (10, 20, 40):
            C1 = _np(sq.scan_tensors(q, keys, nkeys, k=factor_k1, refine_k=0)[1])
            unref = _np(sq.scan_tensors(q, keys, nkeys, k=k, refine_k=0)[1])
            ref = _np(sq.scan_tensors(q, keys, nkeys, k=k, refine_k=factor_k1)[1])
            for qi in range(Q):
                f = set(F[qi][F[qi] >= 0].tolist())
                r, u, c = (len(f & set(a[qi][a[qi] >= 0].tolist())) for a in (ref, unref, C1))
                assert r >= u and r == c, (metric, factor_k1, qi, r, u, c)
                gained += r - u
        assert gained >= 0


# ------------------------------------------------------------------------------------------------ 8. mutation
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_add_and_remove_keep_the_store_in_step(metric):
    from nlsh_amd.indexer import Indexer
    rng = np.random.default_rng(12)
    d, N, M, Q, k = 20, 900, 300, 16, 10
    rows = rng.standard_normal((N + M, d)).astype(np.float32)
    queries = (rows[rng.integers(0, N + M, Q)] + 0.2 * rng.standard_normal((Q, d))).astype(np.float32)
    ckeys = rng.integers(0, 12, size=N + M).astype(np.int32)
    hashing = _hasher(d)
    q = dev(queries)
    qkeys = dev(np.stack([rng.choice(12, 4, replace=False) for _ in range(Q)]).astype(np.int32))
    nkeys = torch.full((Q,), 4, dtype=torch.int32, device="cuda")
    base = dict(compat=False, storage="sq8", refine="device", id_base=50)
    ix = Indexer(hashing, dev(rows[:N]), _dist(metric), corpus_keys=dev(ckeys[:N]), **base)
    quant = tuple(t.clone() for t in ix.quantiser)
    fresh = Indexer(hashing, dev(rows), _dist(metric), corpus_keys=dev(ckeys), quantiser=quant, **base)

    def same(a, b, what):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), what

    # add(ids=...) raises and changes nothing
    gen, held = ix.generation, ix.refine_store.n_rows
    with pytest.raises(ValueError, match="ids"):
        ix.add(dev(rows[N:]), ids=torch.arange(5000, 5000 + M, dtype=torch.int32, device="cuda"), keys=dev(ckeys[N:]))
    assert ix.generation == gen and ix.refine_store.n_rows == held and int(ix.gid.shape[0]) == N
    # add: the fresh index over all rows
    ids = ix.add(dev(rows[N:]), keys=dev(ckeys[N:]))
    assert ids.tolist() == list(range(50 + N, 50 + N + M)) and ix.refine_store.n_rows == N + M
    same(ix.scan_tensors(q, qkeys, nkeys, k=k, want_keys=True), fresh.scan_tensors(q, qkeys, nkeys, k=k, want_keys=True), "add")
    same((ix.refine_store.rows, ix.refine_store.inv_norm) if metric == "cosine" else (ix.refine_store.rows,),
         (fresh.refine_store.rows, fresh.refine_store.inv_norm) if metric == "cosine" else (fresh.refine_store.rows,), "store after add")
    # remove: the fresh index behind a filter that denies the removed ids (word for word the index over the allowed rows)
    gone = (50 + rng.choice(N + M, 200, replace=False)).tolist()
    assert ix.remove(gone) == 200 and ix.refine_store.n_rows == N + M      # the store is left alone
    deny = fresh.row_filter(deny=gone)
    got = ix.scan_tensors(q, qkeys, nkeys, k=k, want_keys=True)
    want = fresh.scan_tensors(q, qkeys, nkeys, k=k, want_keys=True, filter=deny)
    same((got[0], got[1], got[3]), (want[0], want[1], want[3]), "remove")
    assert not np.isin(_np(got[1]), gone).any()
    # both in one call, then once more: the ids go on where the store ends
    more = rng.standard_normal((40, d)).astype(np.float32)
    mkeys = rng.integers(0, 12, size=40).astype(np.int32)
    gone2 = (50 + rng.choice(N + M, 100, replace=False)).tolist()
    new_ids, _ = ix.update(add=dev(more), add_keys=dev(mkeys), remove=gone2)
    assert new_ids.tolist() == list(range(50 + N + M, 50 + N + M + 40)) and ix.refine_store.n_rows == N + M + 40
    fresh2 = Indexer(hashing, dev(np.concatenate([rows, more])), _dist(metric), corpus_keys=dev(np.concatenate([ckeys, mkeys])), quantiser=quant, **base)
    deny2 = fresh2.row_filter(deny=gone + gone2)
    got = ix.scan_tensors(q, qkeys, nkeys, k=k, want_keys=True)
    want = fresh2.scan_tensors(q, qkeys, nkeys, k=k, want_keys=True, filter=deny2)
    same((got[0], got[1], got[3]), (want[0], want[1], want[3]), "update")


# ------------------------------------------------------------------------------------------------ 9. multi-table
@pytest.mark.parametrize("T", [1, 2, 4])
def test_multi_table_reranks_its_merged_lists_once(T):
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.multitable import MultiTableIndexer
    w = _facade_world("sq8", "l2")
    hashers = [_hasher(D_F, H=H_F, seed=77 + 13 * t) for t in range(T)]
    mt = MultiTableIndexer(hashers, dev(w["rows"]), _dist("l2"), storage="sq8", refine="device")
    assert all(t.refine_store is None for t in mt.tables) and mt.refine_store.n_rows == N_F      # ONE store
    q = dev(w["queries"])
    for k in (1, 10, 64):
        k1 = min(256, 4 * k)
        kw = dict(hash_times=4, probes="ranked")
        _, i1, nc1 = mt.query_tensors(q, k=k1, refine_k=0, **kw)
        dist, idx, nc, keys = mt.query_tensors(q, k=k, want_keys=True, **kw)
        rd, ri, rk, _, fb = rerank_reference(w["bits"], _np(i1), k, 0)
        assert fb == -1 and np.array_equal(_np(idx), ri) and np.array_equal(_np(dist).view(np.uint32), rd.view(np.uint32))
        assert np.array_equal(_np(keys).view(np.uint64), rk) and torch.equal(nc, nc1)
        if T == 1:
            single = Indexer(hashers[0], dev(w["rows"]), _dist("l2"), compat=False, algo="tiled", storage="sq8", refine="device")
            sd, si, sn, sk = single.query_tensors(q, k=k, want_keys=True, **kw)
            assert torch.equal(si, idx) and torch.equal(sd.view(torch.int32), dist.view(torch.int32)) and torch.equal(sk, keys) and torch.equal(sn, nc)
    lists, counts = mt.query(q, k=10, hash_times=4, probes="ranked")
    assert [len(r) for r in lists] == (_np(mt.query_tensors(q, k=10, hash_times=4, probes="ranked")[1]) >= 0).sum(1).tolist()
    # add appends once; custom ids are refused
    extra = dev(w["rows"][:7] + np.float32(0.25))
    with pytest.raises(ValueError, match="ids"):
        mt.add(extra, ids=list(range(9000, 9007)))
    assert mt.add(extra).tolist() == list(range(N_F, N_F + 7)) and mt.refine_store.n_rows == N_F + 7
    assert torch.equal(mt.refine_store.rows[N_F:, :D_F], extra)


# ------------------------------------------------------------------------------------------------ 10. host store
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_a_host_store_gives_the_device_stores_words(metric):
    d, kc, k = 100, 70, 10
    w = _world(d, metric)
    rng = np.random.default_rng(6)
    cand = _lists(rng, Q_PURE, kc, 0, N_PURE)
    cand[2, 5] = -1
    host = _store(w["rows"], metric, where="host")
    assert host.rows.is_pinned() and not host.rows.is_cuda and host.n_rows == N_PURE
    assert torch.equal(host.rows, w["store"].rows.cpu())
    got = call_rerank(host, dev(w["queries"]), dev(cand), kc, k)
    ref = call_rerank(w["store"], dev(w["queries"]), dev(cand), kc, k)
    for a, b in zip(got[:4], ref[:4]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert_is_the_reference(got, w["bits"], cand, k, 0, "host store")
    host.append(dev(w["rows"][:5]))
    assert host.n_rows == N_PURE + 5 and torch.equal(host.rows[N_PURE:], w["store"].rows[:5].cpu())


def test_a_device_pointer_passed_as_a_host_store_is_refused():
    w = _world(100, "l2")
    cand = dev(_lists(np.random.default_rng(1), Q_PURE, 10, 0, N_PURE))
    with pytest.raises(_capi.NlshHipError, match="store_on_host"):
        call_rerank(w["store"], dev(w["queries"]), cand, 10, 10, on_host=1)
