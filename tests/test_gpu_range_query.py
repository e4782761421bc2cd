"""Radius queries against THEIR DEFINITION: every candidate of a query with `dist <= radius[q]` (IEEE float32), each once, in the order
of the 64-bit sort key, with the distance bits of the top-k path.  The reference is always the existing top-k path, never the code
under test: (A) a twin index over the same rows and ids whose buckets are cut into chunks of at most 256 rows with fresh keys, scanned
one (probe column, chunk) at a time with `scan_tensors(k=256, want_keys=True)` -- every such call has at most 256 candidates, so the union
of the lists leaves nothing out -- cut by `dist <= r` in numpy float32 and sorted by key; (B) for queries of at most 256 candidates, the
`dist <= r` prefix of the same index's own k = 256 list.  Every comparison is `array_equal` on raw bits.  The shape world is that of
tests/test_gpu_row_filter.py."""
import numpy as np
import pytest
import torch

from helpers import dev
from nlsh_amd import _capi
from test_gpu_corpus_storage import _dist, _hasher
from test_gpu_row_filter import SD, WINDOWS, _assert_task_shapes, _facade_world, _index, _world
from test_range_query_cpu import range_reference

pytestmark = pytest.mark.gpu

FRESH = 10000
_refs = {}


def _fresh(key, c):
    return FRESH + (int(key) + 200) * 4 + c         # the world's keys are 3 b - 200: distinct per (bucket, chunk), none of them a world key


def _reference(storage, form):
    """Reference A of one (storage, metric form): per query the (dist, ids, keys64) of ALL its candidates, sorted by key, and the
    candidate counts of the unchunked top-k call.  Computed once, never written to."""
    if (storage, form) in _refs:
        return _refs[(storage, form)]
    w = _world("uint8" if storage == "uint8" else "float16")
    ck = w["corpus_keys"]
    new, n_chunks = np.empty_like(ck), {}
    for key in np.unique(ck).tolist():
        rows = np.flatnonzero(ck == key)
        n_chunks[key] = (len(rows) + 255) // 256
        for c in range(n_chunks[key]):
            new[rows[c * 256:(c + 1) * 256]] = _fresh(key, c)
    twin = _index(dict(w, corpus_keys=new), storage, form)
    kh, nh = w["keys"].cpu().numpy(), w["nkeys"].cpu().numpy()
    Q, P = kh.shape
    parts = [[] for _ in range(Q)]
    for p in range(P):
        for c in range(max(n_chunks.values())):
            col, cnt = np.zeros((Q, 1), np.int32), np.zeros((Q,), np.int32)
            for qi in range(Q):
                if p < nh[qi] and n_chunks.get(int(kh[qi, p]), 0) > c:
                    col[qi, 0], cnt[qi] = _fresh(kh[qi, p], c), 1
            if not cnt.any():
                continue
            d, i, nc, k64 = twin.scan_tensors(w["q"], dev(col), dev(cnt), k=256, want_keys=True)
            assert int(nc.max()) <= 256, "a condition of the test: the reference leaves nothing out"
            dh, ih, k64h, nch = d.cpu().numpy(), i.cpu().numpy(), k64.cpu().numpy(), nc.cpu().numpy()
            for qi in np.flatnonzero(cnt).tolist():
                m = k64h[qi] != -1
                assert int(m.sum()) == int(nch[qi])
                parts[qi].append((dh[qi][m], ih[qi][m], k64h[qi][m].view(np.uint64)))
    ref = []
    for qi in range(Q):
        if parts[qi]:
            d, i, k = (np.concatenate([x[j] for x in parts[qi]]) for j in range(3))
        else:
            d, i, k = np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint64)
        order = np.argsort(k, kind="stable")
        assert len(np.unique(k)) == len(k)
        ref.append((d[order], i[order], k[order]))
    ix = _index(w, storage, form)
    ix.window_rows = 0
    ncand = ix.scan_tensors(w["q"], w["keys"], w["nkeys"], k=10)[2].cpu().numpy()
    _assert_task_shapes(ix, w)
    assert np.array_equal(ncand, [len(r[0]) for r in ref])
    _refs[(storage, form)] = (w, ix, ref, ncand)
    return _refs[(storage, form)]


def _expected(ref, rad, allowed=None):
    off, ids, dist, keys = [0], [], [], []
    for (d, i, k), r in zip(ref, rad):
        sel = slice(None) if allowed is None else np.isin(i, allowed)
        gi, gd, gk = range_reference(d[sel], i[sel], r)
        assert np.array_equal(gk, k[sel][:len(gk)])       # the cut of a key-sorted list is a prefix of it but for NaN distances (none here)
        ids.append(gi), dist.append(gd), keys.append(gk), off.append(off[-1] + len(gi))
    return np.asarray(off, np.int64), np.concatenate(ids), np.concatenate(dist), np.concatenate(keys)


def _assert_equal(got, want, ncand, what):
    offsets, idx, dist, nc, k64 = got
    assert offsets.dtype == torch.int64 and idx.dtype == torch.int32 and dist.dtype == torch.float32 and nc.dtype == torch.int32, what
    assert all(t.is_cuda for t in (offsets, idx, dist, nc)), what
    print(what, "T =", int(want[0][-1]), "got", int(offsets[-1]))
    assert np.array_equal(offsets.cpu().numpy(), want[0]), (what, "offsets")
    assert np.array_equal(idx.cpu().numpy(), want[1]), (what, "idx")
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), want[2].view(np.uint32)), (what, "distance bits")
    if k64 is not None:
        assert k64.dtype == torch.int64 and np.array_equal(k64.cpu().numpy().view(np.uint64), want[3]), (what, "keys64")
    assert np.array_equal(nc.cpu().numpy(), ncand), (what, "ncand is the top-k call's")


def _radii(ref):
    """name -> float32 [Q], drawn from the reference's own distances."""
    Q = len(ref)
    mth = np.asarray([r[0][len(r[0]) // 2] if len(r[0]) else 0.0 for r in ref], np.float32)
    lo = np.asarray([r[0][0] if len(r[0]) else 0.0 for r in ref], np.float32)
    down = lambda x: np.nextafter(x, np.float32(-np.inf)).astype(np.float32)     # noqa: E731
    return {"m-th distance": mth, "below the m-th": down(mth), "the minimum": lo, "below the minimum": down(lo),
            "zero": np.zeros(Q, np.float32), "minus one": np.full(Q, -1, np.float32), "+inf": np.full(Q, np.inf, np.float32)}


def _range(ix, w, rad, **kw):
    return ix.range_scan_tensors(w["q"], w["keys"], w["nkeys"], dev(rad) if isinstance(rad, np.ndarray) else rad, want_keys=True, **kw)


@pytest.mark.parametrize("storage", ["float32", "float16", "uint8"])
@pytest.mark.parametrize("form", ["l2", "folded", "cosine"])
def test_range_scan_equals_the_chunked_twin_on_every_task_shape(form, storage):
    w, ix, ref, ncand = _reference(storage, form)
    radii = _radii(ref)
    ties = [qi for qi, r in enumerate(ref) if len(r[0]) > 1 and np.any(r[0][1:] == r[0][:-1])]
    assert ties, "mass ties exist"
    n_in = {name: sum(int((r[0] <= rad[qi]).sum()) for qi, r in enumerate(ref)) for name, rad in radii.items()}
    assert n_in["+inf"] == int(ncand.sum()) and 0 < n_in["below the m-th"] < n_in["m-th distance"] < n_in["+inf"]
    assert n_in["below the minimum"] == 0 and (form == "cosine" or n_in["minus one"] == 0)
    for window in WINDOWS:
        ix.window_rows = window
        for name, rad in radii.items():
            got = _range(ix, w, rad)
            assert ix.last_window == window and ix.last_algo == _capi.SCAN_BUCKET_TILED
            _assert_equal(got, _expected(ref, rad), ncand, (form, storage, window, name))
    # one scalar radius, and the same call without the keys
    scalar = float(np.median(np.concatenate([r[0] for r in ref])))
    want = _expected(ref, np.full(len(ref), scalar, np.float32))
    assert 0 < want[0][-1] < ncand.sum()
    _assert_equal(_range(ix, w, scalar), want, ncand, (form, storage, "scalar"))
    plain = ix.range_scan_tensors(w["q"], w["keys"], w["nkeys"], scalar)
    assert plain[4] is None
    _assert_equal(plain, want, ncand, (form, storage, "scalar, no keys"))


@pytest.mark.parametrize("storage", ["float32", "float16", "uint8"])
@pytest.mark.parametrize("form", ["l2", "cosine"])
def test_range_scan_behind_a_filter(form, storage):
    w, ix, ref, ncand = _reference(storage, form)
    radii = _radii(ref)
    N = len(w["ids"])
    rng = np.random.default_rng(3)
    for name, local in (("half", rng.random(N) < 0.5), ("all", np.ones(N, bool)), ("none", np.zeros(N, bool))):
        F = ix.row_filter(allow=dev(w["ids"][local]))
        allowed = w["ids"][local]
        for window in (0, 64):
            ix.window_rows = window
            for rname in ("m-th distance", "+inf"):
                got = _range(ix, w, radii[rname], filter=F)
                want = _expected(ref, radii[rname], allowed)
                _assert_equal(got, want, ncand, (form, storage, name, window, rname))
                if name == "none":
                    assert got[1].numel() == 0 and not got[0].any()
                if name == "all":
                    _assert_equal(_range(ix, w, radii[rname]), want, ncand, (form, storage, "unfiltered", window, rname))


@pytest.mark.parametrize("storage", ["float32", "uint8"])
def test_range_scan_equals_the_prefix_of_the_own_wide_list(storage):
    """Reference B: the same index, the same task table."""
    w, ix, ref, ncand = _reference(storage, "l2")
    light = np.flatnonzero(ncand <= 256)
    assert set(w["light"]) <= set(light.tolist())
    for window in (0, 64):
        ix.window_rows = window
        wd, wi, _, wk = (t.cpu().numpy() for t in ix.scan_tensors(w["q"], w["keys"], w["nkeys"], k=256, want_keys=True))
        for name, rad in _radii(ref).items():
            off, idx, dist, _, k64 = (t.cpu().numpy() for t in _range(ix, w, rad))
            for qi in light.tolist():
                with np.errstate(invalid="ignore"):
                    keep = (wk[qi] != -1) & (wd[qi] <= rad[qi])
                lo, hi = off[qi], off[qi + 1]
                assert np.array_equal(idx[lo:hi], wi[qi][keep]) and np.array_equal(k64[lo:hi], wk[qi][keep]), (storage, window, name, qi)
                assert np.array_equal(dist[lo:hi].view(np.uint32), wd[qi][keep].view(np.uint32))


# ---------------------------------------------------------------------------------------------- non-finite rows
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_non_finite_rows(metric):
    from nlsh_amd.indexer import Indexer
    rng = np.random.default_rng(8)
    N, d = 300, 12
    V = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    nan_rows, inf_rows = [5, 70, 299], [9, 130]
    V[nan_rows, 3] = np.nan
    V[nan_rows[1]] = np.nan
    if metric == "l2":
        V[inf_rows] = 3e30                                          # (q - c)^2 overflows float32: a distance of +inf
    ids = np.arange(N, dtype=np.int32) * 2 + 100
    ck = np.where(np.arange(N) < 280, 5, 6).astype(np.int32)       # one bucket of two segments, one small one
    ix = Indexer(_hasher(d), dev(V), _dist(metric), compat=False, algo="tiled", row_ids=dev(ids), corpus_keys=dev(ck))
    q = dev(rng.integers(-3, 4, size=(3, d)).astype(np.float32) + 0.5)
    key_lists = [[5, 6], [6], [5]]
    cand = [np.arange(N), np.arange(280, N), np.arange(280)]
    for window in (0, 64):
        ix.window_rows = window
        rows, nc, dists = ix.range_query_with_keys(q, key_lists, float("inf"), return_distances=True)
        assert nc == [len(c) for c in cand]
        for qi in range(3):
            want = set(int(ids[c]) for c in cand[qi] if c not in nan_rows)
            assert set(rows[qi]) == want and len(rows[qi]) == len(want), "a NaN row is absent even at +inf"
            assert not np.isnan(dists[qi]).any() and dists[qi] == sorted(dists[qi])
            if metric == "l2":
                n_inf = sum(1 for c in cand[qi] if c in inf_rows)
                assert [int(ids[c]) for c in inf_rows if c in cand[qi]] == rows[qi][len(rows[qi]) - n_inf:], "+inf distances come last, by id"
                assert all(np.isinf(x) for x in dists[qi][len(dists[qi]) - n_inf:])
        if metric == "l2":
            rows_big, _ = ix.range_query_with_keys(q, key_lists, 3.0e38)
            for qi in range(3):
                assert set(rows_big[qi]) == set(int(ids[c]) for c in cand[qi] if c not in nan_rows and c not in inf_rows), "+inf only at +inf"
            assert ix.range_query_with_keys(q, key_lists, -1.0)[0] == [[], [], []]


# ---------------------------------------------------------------------------------------------- the table, the edges, the limit
def test_task_table_overflow_empty_batches_and_limit():
    w, ix, ref, ncand = _reference("float32", "l2")
    radii = _radii(ref)
    ix.window_rows = 0
    rad = radii["m-th distance"]
    want = _expected(ref, rad)
    first = _range(ix, w, rad)
    _assert_equal(first, want, ncand, "before")
    tkey = ix._tkey(_capi.SCAN_BUCKET_TILED, w["Q"], w["P"])
    needed = int(ix.last_status.cpu()[0])
    ix._max_tasks[tkey] = 4                                            # a table of a few tasks: the count call flags it, the facade retries
    again = _range(ix, w, rad)
    assert ix._last_max_tasks >= needed > 4 and int(ix.last_status.cpu()[1]) == 0
    _assert_equal(again, want, ncand, "after the retry")
    for a, b in zip(first, _range(ix, w, rad)):                        # repeated calls: identical bits
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    # Q = 0
    off, idx, dist, nc, k64 = ix.range_scan_tensors(w["q"][:0], w["keys"][:0], w["nkeys"][:0], 1.0, want_keys=True)
    assert off.tolist() == [0] and idx.numel() == dist.numel() == nc.numel() == k64.numel() == 0
    # nothing in range anywhere
    off, idx, dist, nc, k64 = _range(ix, w, radii["below the minimum"])
    assert off.tolist() == [0] * (w["Q"] + 1) and idx.numel() == dist.numel() == k64.numel() == 0 and np.array_equal(nc.cpu().numpy(), ncand)
    # an all-unknown key table
    off, idx, dist, nc, k64 = ix.range_scan_tensors(w["q"], torch.full_like(w["keys"], 999999), w["nkeys"], float("inf"), want_keys=True)
    assert not off.any() and idx.numel() == 0 and not nc.any()
    # no keys at all
    off, idx, dist, nc, _ = ix.range_scan_tensors(w["q"], w["keys"], torch.zeros_like(w["nkeys"]), float("inf"))
    assert not off.any() and idx.numel() == 0 and not nc.any()
    # limit
    T = int(want[0][-1])
    _assert_equal(_range(ix, w, rad, limit=T), want, ncand, "limit == T")
    with pytest.raises(ValueError, match="limit"):
        _range(ix, w, rad, limit=T - 1)
    with pytest.raises(ValueError, match="limit"):
        _range(ix, w, rad, limit=0)
    with pytest.raises(ValueError, match="NaN"):
        _range(ix, w, np.full(w["Q"], np.nan, np.float32))
    with pytest.raises(ValueError, match="is on"):
        ix.range_scan_tensors(w["q"], w["keys"], w["nkeys"], torch.zeros(w["Q"]))


def test_raw_calls_leave_the_words_behind_their_outputs_alone():
    """`nlsh_range_count` / `nlsh_range_fill` themselves, with canary words behind out_count, out_ncand, cursor, out_keys, out_dist and
    out_idx, on a workspace sized by `nlsh_range_workspace`; and with out_keys / out_dist not wanted."""
    w, ix, ref, ncand = _reference("float32", "l2")
    L, stream, Q, P, pad, canary = _capi.lib(), torch.cuda.current_stream().cuda_stream, w["Q"], w["P"], 8, 0x5A5A5A5A
    rad_h = _radii(ref)["m-th distance"]
    rad, want = dev(rad_h), _expected(ref, rad_h)
    T = int(want[0][-1])
    for window in (0, 64):
        ix.window_rows = window
        _range(ix, w, rad_h)                                            # settles the task table of this shape
        max_tasks = ix._last_max_tasks
        head = ix._range_head(w["q"], w["keys"], w["nkeys"], window, None, rad)
        ws = torch.zeros((L.nlsh_range_workspace(Q, P, max_tasks, ix.n_buckets, SD),), dtype=torch.uint8, device="cuda")
        count, nc = (torch.full((Q + pad,), canary, dtype=torch.int32, device="cuda") for _ in range(2))
        status = torch.zeros((2,), dtype=torch.int32, device="cuda")
        tail = (status.data_ptr(), ws.data_ptr(), ws.numel(), max_tasks)
        _capi.check(L.nlsh_range_count(*head, count.data_ptr(), nc.data_ptr(), *tail, None, None, stream))
        assert status.cpu().tolist()[1] == 0
        ch, nh = count.cpu().numpy(), nc.cpu().numpy()
        assert np.array_equal(ch[:Q], np.diff(want[0])) and np.all(ch[Q:] == canary)
        assert np.array_equal(nh[:Q], ncand) and np.all(nh[Q:] == canary)
        offsets = dev(want[0])
        for with_keys, with_dist in ((True, True), (False, False)):
            cursor = torch.full((Q + pad,), canary, dtype=torch.int32, device="cuda")
            idx = torch.full((T + pad,), canary, dtype=torch.int32, device="cuda")
            dist = torch.full((T + pad,), canary, dtype=torch.int32, device="cuda")
            k64 = torch.full((T + pad,), canary, dtype=torch.int64, device="cuda")
            sb = L.nlsh_range_sort_workspace(Q, T)
            sws = torch.empty((sb,), dtype=torch.uint8, device="cuda")
            _capi.check(L.nlsh_range_fill(*head, offsets.data_ptr(), T, cursor.data_ptr(), k64.data_ptr() if with_keys else None,
                                          dist.data_ptr() if with_dist else None, idx.data_ptr(), *tail, sws.data_ptr(), sb, None, None, stream))
            cu, ih, dh, kh = cursor.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy(), k64.cpu().numpy()
            assert np.array_equal(cu[:Q], np.diff(want[0])) and np.all(cu[Q:] == canary)
            assert np.array_equal(ih[:T], want[1]) and np.all(ih[T:] == canary)
            assert np.array_equal(dh[:T].view(np.uint32), want[2].view(np.uint32)) if with_dist else np.all(dh[:T] == canary)
            assert np.all(dh[T:] == canary)
            assert np.array_equal(kh[:T].view(np.uint64), want[3]) if with_keys else np.all(kh[:T] == canary)
            assert np.all(kh[T:] == canary)
    # the sort workspace's bound holds rocPRIM's own need at every size tried (the fill call checks it before it launches anything)
    got = [L.nlsh_range_sort_workspace(64, t) for t in (0, 1, 255, 256, 257, 10 ** 4, 10 ** 6)]
    assert all(a <= b for a, b in zip(got, got[1:])) and got[0] > 0


# ---------------------------------------------------------------------------------------------- facade
def test_range_query_routes_equal_the_wide_top_k_lists():
    """`range_tensors` / `range_query` / `range_query_with_keys` on hashed keys -- sampled, ranked, ranked with a candidate budget --
    against the index's own k = 256 `query_tensors` of the same call on the queries of at most 256 candidates (Reference B)."""
    rng, V, ids, hashing, ix, q = _facade_world(seed=31)
    checked = 0
    for kw in (dict(hash_times=10, seed=5), dict(hash_times=12, probes="ranked"), dict(hash_times=16, probes="ranked", candidate_budget=40),
               dict(hash_times=1, seed=7)):
        wd, wi, wn, wk = (t.cpu().numpy() for t in ix.query_tensors(q, k=256, want_keys=True, **kw))
        finite = wd[wk != -1]
        radius = float(np.quantile(finite, 0.3))
        off, idx, dist, nc, k64 = ix.range_tensors(q, radius, want_keys=True, **kw)
        assert ix.last_query_path == "two_step" and ix.last_algo == _capi.SCAN_BUCKET_TILED
        oh, ih, dh, kh = off.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy(), k64.cpu().numpy()
        assert np.array_equal(nc.cpu().numpy(), wn), kw
        for qi in np.flatnonzero(wn <= 256).tolist():
            keep = (wk[qi] != -1) & (wd[qi] <= np.float32(radius))
            lo, hi = oh[qi], oh[qi + 1]
            assert np.array_equal(ih[lo:hi], wi[qi][keep]) and np.array_equal(kh[lo:hi], wk[qi][keep]), (kw, qi)
            assert np.array_equal(dh[lo:hi].view(np.uint32), wd[qi][keep].view(np.uint32))
            checked += int(keep.sum())
        rows, counts, dists = ix.range_query(q, radius, return_distances=True, **kw)
        assert rows == [ih[a:b].tolist() for a, b in zip(oh[:-1], oh[1:])] and counts == wn.tolist()
        assert dists == [dh[a:b].tolist() for a, b in zip(oh[:-1], oh[1:])]
        assert ix.range_query(q, radius, **kw) == (rows, counts)
        if "seed" in kw:
            keys, nkeys = ix.hash_device(q, **kw)
            kl, nl = keys.cpu().numpy(), nkeys.cpu().numpy()
            key_lists = [[int(v) & 0xFFFFFFFF for v in kl[i, :nl[i]]] for i in range(len(nl))]
            assert ix.range_query_with_keys(q, key_lists, radius, return_distances=True) == (rows, counts, dists)
    assert checked > 100
    # per-query radii through the hashed route, and a filter
    rad = dev(np.where(np.arange(q.shape[0]) % 2, np.float32(np.inf), np.float32(-1.0)).astype(np.float32))
    off, idx, dist, nc, _ = ix.range_tensors(q, rad, hash_times=10, seed=5)
    assert np.array_equal(np.diff(off.cpu().numpy()), np.where(np.arange(q.shape[0]) % 2, nc.cpu().numpy(), 0))
    local = rng.random(len(ids)) < 0.5
    F = ix.row_filter(allow=dev(ids[local]))
    rows, _ = ix.range_query(q, float("inf"), hash_times=10, seed=5, filter=F)
    full, _ = ix.range_query(q, float("inf"), hash_times=10, seed=5)
    allowed = set(ids[local].tolist())
    assert rows == [[i for i in r if i in allowed] for r in full] and any(rows)
    with pytest.raises(ValueError, match="hash_times"):
        ix.range_tensors(q, 1.0, hash_times=65)
    ix.add(dev(rng.standard_normal((5, V.shape[1])).astype(np.float32)), ids=dev(np.arange(-5, 0, dtype=np.int32)))
    with pytest.raises(ValueError, match="stale"):
        ix.range_query(q, 1.0, filter=F)
