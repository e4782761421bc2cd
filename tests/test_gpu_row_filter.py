"""Filtered queries against THEIR DEFINITION: a call on index I with filter F gives, word for word, what the same call gives on the
index I_F built by the existing constructor from the allowed rows alone (`row_ids=`, `corpus_keys=`, `compat=False`, the same query key
table) -- ids, distance bits and the 64-bit sort keys, padding included -- while the candidate counts stay the unfiltered call's.
The reference is always the unfiltered path on another index (or, second angle, the same index's own unfiltered k = 256 result
post-filtered on the host), never the code under test; every comparison is `torch.equal` / `array_equal` on raw bits.  The filter
words are held against the numpy packing rule of tests/test_row_filter_cpu.py."""
import numpy as np
import pytest
import torch

from helpers import dev
from helpers import task_table as _task_table
from nlsh_amd import _capi
from test_gpu_corpus_storage import _dist, _hasher, _same, queries_for, stored
from test_row_filter_cpu import pack_loop

pytestmark = pytest.mark.gpu

TORCH = {"float32": torch.float32, "float16": torch.float16, "uint8": torch.uint8}
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _pack(allowed):
    from nlsh_amd.indexer import pack_row_filter
    return pack_row_filter(allowed)


def _words(F):
    return F.words.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------- filter build against numpy
def _id_layouts(N, rng):
    """name -> (row_ids or None, id_base)."""
    out = {"dense from -50": (None, -50)}
    if N:
        sparse = np.sort(rng.choice(np.arange(-3 * N - 7, 3 * N + 7), size=N, replace=False)).astype(np.int64)
        out["sparse, negative"] = (rng.permutation(sparse).astype(np.int32), 0)
        edge = sparse.copy()
        edge[0] = I32_MIN
        if N > 1:
            edge[-1] = I32_MAX
        out["int32 limits"] = (rng.permutation(edge).astype(np.int32), 0)
    return out


def _tiny_index(N, row_ids, id_base, rng):
    from nlsh_amd.indexer import Indexer
    keys = dev(rng.integers(-3, 4, size=N).astype(np.int32))
    return Indexer(_hasher(4), dev(rng.standard_normal((N, 4)).astype(np.float32)), _dist("l2"), corpus_keys=keys, compat=False,
                   id_base=id_base, row_ids=None if row_ids is None else dev(row_ids))


def _check_filter(F, gid, allowed_ids, invert, what):
    member = np.isin(gid, np.asarray(list(allowed_ids), dtype=np.int64))
    allowed = member != invert
    got, want = _words(F), _pack(allowed)
    assert got.shape == want.shape and np.array_equal(got, want), what
    assert np.array_equal(want, pack_loop(allowed))
    assert F.n_allowed == int(allowed.sum()), what
    n = len(gid)
    if n % 64:          # the tail bits are zero
        tail = np.unpackbits(got.view(np.uint8), bitorder="little")[n:]
        assert not tail.any(), what


@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 64, 65, 20000])
def test_filter_words_equal_numpy(N):
    rng = np.random.default_rng(N)
    for name, (row_ids, id_base) in _id_layouts(N, rng).items():
        ix = _tiny_index(N, row_ids, id_base, rng)
        gid = ix.gid.cpu().numpy().astype(np.int64)
        assert len(gid) == N
        ids = np.unique(gid)
        half = rng.choice(ids, size=max(1, N // 2), replace=False)
        unknown = np.asarray([v for v in (I32_MIN + 1, -7 * N - 100, 7 * N + 100, I32_MAX - 1) if v not in set(ids.tolist())], dtype=np.int64)
        cases = {
            "half": half, "all": ids, "empty": np.zeros(0, np.int64), "unknown only": unknown,
            "duplicates + unknown": np.r_[half, half[::-1], unknown, half[:3]], "first and last sorted row": gid[[0, -1]],
            "outside int32": np.r_[half, 1 << 40, -(1 << 40)],
        }
        for cname, given in cases.items():
            for form in (list(given.tolist()), dev(given.astype(np.int64)), dev(np.repeat(given.astype(np.int64), 2))[::2]):
                _check_filter(ix.row_filter(allow=form), gid, given, False, (name, cname, "allow"))
                _check_filter(ix.row_filter(deny=form), gid, given, True, (name, cname, "deny"))
        _check_filter(ix.row_filter(allow=dev(half.astype(np.int32))), gid, half, False, (name, "int32 tensor"))
        # masks are indexed by id - id_base; ids outside the mask (negative offsets, a mask shorter than the id range) are denied
        span = int(gid.max()) - id_base + 1
        if 0 < span <= 1 << 20:
            for length in (span, max(span // 2, 1), span + 9, 0):
                m = rng.random(length) < 0.5
                off = gid - id_base
                inside = (off >= 0) & (off < length)
                want_ids = gid[inside][m[off[inside]]] if length else np.zeros(0, np.int64)
                for t in (dev(m), dev(m.astype(np.uint8)), dev(m.astype(np.uint8) * 200)):
                    _check_filter(ix.row_filter(mask=t), gid, want_ids, False, (name, "mask", length, t.dtype))


def test_filter_build_call_on_raw_ids():
    """`nlsh_row_filter_build` itself, N = 0 included (no index of zero rows is built): both sources, both polarities."""
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(1)
    for N in (0, 1, 63, 64, 65, 1000):
        gid = rng.permutation(np.arange(-N, N, 2))[:N].astype(np.int32) if N else np.zeros(0, np.int32)
        ids = np.unique(rng.choice(np.arange(-N - 5, N + 5), size=N // 2 + 1)).astype(np.int32)
        dense = (rng.random(N + 3) < 0.5).astype(np.uint8)
        g, words = dev(gid), torch.full((int(L.nlsh_row_filter_words(N)) + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        n_allowed = torch.full((1,), -9, dtype=torch.int32, device="cuda")
        ids_d, dense_d, base = dev(ids), dev(dense), -(N // 2)
        for invert in (0, 1):
            for src, want in (((ids_d.data_ptr(), len(ids), None, 0, 0), np.isin(gid, ids)),
                              ((None, 0, dense_d.data_ptr(), len(dense), base),
                               np.asarray([0 <= int(v) - base < len(dense) and dense[int(v) - base] != 0 for v in gid], dtype=bool))):
                _capi.check(L.nlsh_row_filter_build(g.data_ptr() if N else None, N, *src, invert, words.data_ptr(), n_allowed.data_ptr(), stream))
                allowed = want != bool(invert)
                got = words.cpu().numpy().view(np.uint32)
                assert np.array_equal(got[:-2], _pack(allowed)) and np.all(got[-2:] == 0x5A5A5A5A), (N, invert)     # nothing written behind the words
                assert int(n_allowed.item()) == int(allowed.sum())


# ---------------------------------------------------------------------------------------------- scan on every task shape
SIZES = (1, 2, 40, 41, 63, 64, 65, 255, 256, 257, 700)   # rows per bucket: single-stage tasks either side of rows * d4 <= 1024 (d = 100), 1..4 tiles, 2 and 3 segments
GROUPS = (1, 5, 11, 16, 17)                               # queries per bucket: a wave holds 1,0 / 2,1 / 3,2 / 4 of them; 17 = two groups
TINY = 48                                                 # a run of buckets of 1..6 rows: shared windows
LIGHT = ((65, 1), (130, 2), (200, 1), (255, 2), (30, 2))  # buckets probed by the LIGHT queries alone: <= 256 candidates per query, 2..4-tile tasks among them
SD, SQ, NLIGHT = 100, 64, 8
KS = (1, 10, 64, 65, 100, 256)
WINDOWS = (0, 64, 128, 256)
_worlds = {}


def _world(kind):
    """`_shape_world` of tests/test_gpu_corpus_storage.py (kind: "float16" values, which the float32 index holds as float32, or "uint8")
    plus NLIGHT queries of few candidates and row ids that are sparse and partly negative.  Computed once, never written to."""
    if kind in _worlds:
        return _worlds[kind]
    rng = np.random.default_rng(77 + len(kind))
    buckets = [(s, m) for s in SIZES for m in GROUPS] + [(1 + i % 6, 1 + i % 3) for i in range(TINY)] + list(LIGHT)
    N = sum(s for s, _ in buckets)
    S = stored(kind, N, SD, rng)
    bkey = lambda b: int(b * 3 - 200)       # noqa: E731
    keys = np.repeat(np.asarray([bkey(b) for b in range(len(buckets))], dtype=np.int32), [s for s, _ in buckets])
    order = rng.permutation(N)
    corpus_keys = np.empty(N, np.int32)
    corpus_keys[order] = keys
    rows_of = {b: np.flatnonzero(corpus_keys == bkey(b)) for b in range(len(buckets))}
    ties = next(b for b, (s, m) in enumerate(buckets) if s == 256 and m == 17)
    S[rows_of[ties]] = S[rows_of[ties][0]]                          # a bucket of identical rows: the (distance, id) order decides
    key_lists = [[] for _ in range(SQ + NLIGHT)]
    n_heavy = len(buckets) - len(LIGHT)
    for b, (s, m) in enumerate(buckets[:n_heavy]):
        for qi in rng.choice(SQ, size=m, replace=False):
            key_lists[qi].append(bkey(b))
    li = 0
    for b in range(n_heavy, len(buckets)):
        for _ in range(buckets[b][1]):
            key_lists[SQ + li % NLIGHT].append(bkey(b))
            li += 1
    for qi in range(SQ):
        rng.shuffle(key_lists[qi])
    key_lists[7].insert(1, 999999)                                  # an unknown key
    P = max(len(ks) for ks in key_lists)
    assert P <= _capi.MAX_PROBES
    Q = SQ + NLIGHT
    tab, cnt = np.zeros((Q, P), np.int32), np.zeros((Q,), np.int32)
    for qi, ks in enumerate(key_lists):
        tab[qi, :len(ks)], cnt[qi] = ks, len(ks)
    # sparse ids either side of INT32_MAX / INT32_MIN.  The sort key holds the id as a uint32, so ties come out in UNSIGNED id order
    # (negative ids last); these ids ascend with the local row in that order, which is the order the oracle breaks ties in
    ids = ((1 << 31) - 8001 + 2 * np.arange(N, dtype=np.int64)).astype(np.uint32).view(np.int32)
    assert ids[0] > 0 and ids[-1] < 0
    w = dict(S=S, corpus_keys=corpus_keys, buckets=buckets, rows_of=rows_of, ties=ties, ids=ids, keys=dev(tab), nkeys=dev(cnt),
             q=dev(queries_for(kind, Q, SD, rng)), Q=Q, P=P, light=list(range(SQ, Q)))
    _worlds[kind] = w
    return w


def _index(w, storage, form, local=None, **kw):
    """The index of the world's rows `local` (all by default) in `storage`, built by the constructor."""
    from nlsh_amd.indexer import Indexer
    sel = slice(None) if local is None else local
    rows = dev(w["S"][sel]).to(TORCH[storage])
    metric = "cosine" if form == "cosine" else "l2"
    if form == "folded":
        kw["l2_form"] = "folded"
    return Indexer(_hasher(SD), rows, _dist(metric), storage=storage, algo="tiled", compat=False, row_ids=dev(w["ids"][sel]),
                   corpus_keys=dev(w["corpus_keys"][sel]), **kw)


def _filters(w, ix):
    """name -> bool [N] over the LOCAL rows.  The position-defined ones are stated on the sorted rows and carried over by id."""
    N = len(w["ids"])
    rng = np.random.default_rng(3)
    gid = ix.gid.cpu().numpy()
    by_pos = lambda pos_mask: np.isin(w["ids"], gid[pos_mask])      # noqa: E731
    pos = np.arange(N)
    big = next(b for b, (s, m) in enumerate(w["buckets"]) if s == 700 and m == 16)
    ties_rows = w["rows_of"][w["ties"]]
    out = {
        "all": np.ones(N, bool), "none": np.zeros(N, bool), "last sorted row": by_pos(pos == N - 1),
        "every other sorted row": by_pos(pos % 2 == 0), "half": rng.random(N) < 0.5, "1 %": rng.random(N) < 0.01,
        "one bucket denied": ~np.isin(np.arange(N), w["rows_of"][big]),
        "ties: three left": ~np.isin(np.arange(N), np.setdiff1d(ties_rows, ties_rows[[3, 100, 255]])),
    }
    words = _pack(np.isin(gid, w["ids"][out["every other sorted row"]]))
    assert np.all((words[:N // 32] != 0) & (words[:N // 32] != 0xFFFFFFFF))     # every 32-row word is mixed
    return out


def _raw_equal(a, b, what):
    _same(a[0], b[0], (what, "dist"))
    _same(a[1], b[1], (what, "idx"))
    _same(a[3], b[3], (what, "keys64"))


def _assert_padding(r, what):
    assert bool((r[1] == -1).all()) and bool(torch.isinf(r[0]).all() and (r[0] > 0).all()) and bool((r[3] == -1).all()), what


def _scan(ix, w, k, **kw):
    return ix.scan_tensors(w["q"], w["keys"], w["nkeys"], k=k, want_keys=True, **kw)


def _assert_task_shapes(ix, w):
    """Window 0: every (queries per wave 0..4) x (1..4 tiles) shape and the single-stage body either side of its threshold."""
    nq, nrows = _task_table(ix, w["Q"], w["P"], 10, SD)
    d4 = (SD + 3) // 4
    shapes, single = set(), {True: set(), False: set()}
    for a, r in zip(nq.tolist(), nrows.tolist()):
        per_wave = {max(0, min(4, (a - wave + 3) // 4)) for wave in range(4)}
        shapes |= {(n, (r + 63) // 64) for n in per_wave}
        if r <= 64:
            single[r * d4 <= 1024] |= per_wave
    assert shapes == {(n, t) for n in range(5) for t in range(1, 5)}, sorted(shapes)
    assert single[True] == set(range(5)) and single[False] == set(range(5)), single
    assert {40, 41} <= set(nrows.tolist())
    assert len(nq) == sum(((m + 15) // 16) * ((s + 255) // 256) for s, m in w["buckets"])


@pytest.mark.parametrize("storage", ["float32", "float16", "uint8"])
@pytest.mark.parametrize("form", ["l2", "folded", "cosine"])
def test_filtered_scan_equals_the_twin_on_every_task_shape(form, storage):
    w = _world("uint8" if storage == "uint8" else "float16")
    ix = _index(w, storage, form)
    ix.window_rows = 0
    unfiltered = {(0, 10): _scan(ix, w, 10)}
    _assert_task_shapes(ix, w)
    for window in WINDOWS:
        ix.window_rows = window
        for k in KS:
            unfiltered[(window, k)] = _scan(ix, w, k)
            assert ix.last_window == window
    for name, local in _filters(w, ix).items():
        F = ix.row_filter(allow=dev(w["ids"][local]))
        assert F.n_allowed == int(local.sum()) and F.generation == ix.generation
        twin = _index(w, storage, form, local) if local.any() else None
        if form == "l2" and storage == "float32" and twin is not None:
            oracle_ref = _oracle_lists(w, local, 10)
        for window in WINDOWS:
            ix.window_rows = window
            if twin is not None:
                twin.window_rows = window
            for k in KS:
                what = (form, storage, name, window, k)
                got = _scan(ix, w, k, filter=F)
                assert ix.last_window == window and ix.last_algo == _capi.SCAN_BUCKET_TILED
                _same(got[2], unfiltered[(window, k)][2], (what, "ncand is the unfiltered call's"))
                if twin is None:
                    _assert_padding(got, what)
                else:
                    _raw_equal(got, _scan(twin, w, k), what)
                if name == "all":
                    _raw_equal(got, unfiltered[(window, k)], (what, "against the unfiltered call"))
                if k == 10 and form == "l2" and storage == "float32" and twin is not None:
                    od, oi = oracle_ref
                    assert np.array_equal(got[1].cpu().numpy(), oi), what
                    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), od.view(np.uint32)), what
    # the ties bucket with three rows left: their ids, ascending, lead every list of the bucket's queries that they win
    dist, idx = got[0].cpu().numpy(), got[1].cpu().numpy()
    for row_d, row_i in zip(dist, idx):
        same = (row_d[1:] == row_d[:-1]) & np.isfinite(row_d[1:])
        row_u = row_i.view(np.uint32)                               # the sort key's id word
        assert np.all(row_u[1:][same] > row_u[:-1][same])


def _oracle_lists(w, local, k):
    """The CPU oracle over the allowed rows (exact L2, float32) -> (dist, ids) with the oracle's local rows mapped back to ids."""
    from oracle import oracle
    ox = oracle.OracleIndexer.from_keys(w["S"][local].astype(np.float32), w["corpus_keys"][local])
    kh, nh = w["keys"].cpu().numpy().astype(np.int64), w["nkeys"].cpu().numpy()
    od, oi, _ = oracle.query_batch(ox.corpus, ox.perm, ox.uniq_keys, ox.offsets, w["q"].cpu().numpy(), kh, nh, k, "l2", simd=True)
    ids = w["ids"][local]
    return od, np.where(oi >= 0, ids[np.clip(oi, 0, None)], -1).astype(np.int32)


# ---------------------------------------------------------------------------------------------- second angle: the same index, post-filtered
@pytest.mark.parametrize("storage", ["float32", "float16", "uint8"])
def test_filtered_scan_equals_own_post_filtered_wide_scan(storage):
    """The filter against the SAME task table: for queries of at most 256 candidates the unfiltered k = 256 list holds every candidate
    in (distance, id) order, so dropping the denied ids on the host and cutting to k is the filtered answer."""
    w = _world("uint8" if storage == "uint8" else "float16")
    ix = _index(w, storage, "l2")
    ix.window_rows = 0
    wide = _scan(ix, w, 256)
    tab, qids, _ = _task_table(ix, w["Q"], w["P"], 256, SD, full=True)
    ncand = wide[2].cpu().numpy()
    small = np.flatnonzero(ncand <= 256)
    assert set(w["light"]) <= set(small.tolist())
    multi = {int(qi) for t in range(len(tab)) if tab[t, 3] > 64 for qi in qids[t, :tab[t, 1]]}
    assert multi & set(small.tolist()), "a query of <= 256 candidates must probe a multi-tile task"
    wd, wi, wk = wide[0].cpu().numpy().view(np.uint32), wide[1].cpu().numpy(), wide[3].cpu().numpy()
    for window in (0, 64):
        ix.window_rows = window
        for name, local in _filters(w, ix).items():
            F = ix.row_filter(deny=dev(w["ids"][~local]))
            allowed = set(w["ids"][local].tolist())
            for k in (1, 10, 100):
                got = _scan(ix, w, k, filter=F)
                gd, gi = got[0].cpu().numpy().view(np.uint32), got[1].cpu().numpy()
                for qi in small.tolist():
                    keep = [j for j in range(256) if wk[qi, j] != -1 and int(wi[qi, j]) in allowed][:k]
                    want_i = np.full(k, -1, np.int32)
                    want_d = np.full(k, np.float32(np.inf).view(np.uint32), np.uint32)
                    want_i[:len(keep)], want_d[:len(keep)] = wi[qi, keep], wd[qi, keep]
                    assert np.array_equal(gi[qi], want_i) and np.array_equal(gd[qi], want_d), (storage, name, window, k, qi)


# ---------------------------------------------------------------------------------------------- denied rows cannot poison a list
@pytest.mark.parametrize("storage", ["float32", "float16"])
@pytest.mark.parametrize("form", ["l2", "cosine"])
def test_denied_non_finite_rows_leave_every_list_the_twins(form, storage):
    base = _world("float16")
    w = dict(base, S=base["S"].copy())
    rng = np.random.default_rng(9)
    N = len(w["ids"])
    bad = rng.choice(N, size=N // 8, replace=False)
    vals = np.asarray([np.nan, np.inf, -np.inf], dtype=np.float16)
    w["S"][bad, rng.integers(0, SD, size=len(bad))] = vals[rng.integers(0, 3, size=len(bad))]
    w["S"][bad[:40]] = np.float16(np.nan)                           # whole rows of NaN as well
    ix = _index(w, storage, form)
    deny_bad = ~np.isin(np.arange(N), bad)
    some_bad = deny_bad | np.isin(np.arange(N), bad[::3])           # allowed non-finite rows behave as in the twin
    for name, local in (("bad rows denied", deny_bad), ("a third of the bad rows allowed", some_bad)):
        F = ix.row_filter(allow=dev(w["ids"][local]))
        twin = _index(w, storage, form, local)
        for window in (0, 64, 256):
            ix.window_rows = twin.window_rows = window
            for k in (10, 100):
                got = _scan(ix, w, k, filter=F)
                _raw_equal(got, _scan(twin, w, k), (form, storage, name, window, k))
        if name == "bad rows denied":
            finite = torch.isfinite(got[0]) | (got[1] == -1)
            assert bool(finite.all()), "a denied non-finite row reached a list"


# ---------------------------------------------------------------------------------------------- dimensions
@pytest.mark.parametrize("d", [1, 3, 100, 128, 260, 1024])
def test_filtered_scan_across_dimensions(d):
    from nlsh_amd.indexer import Indexer
    rng = np.random.default_rng(d)
    N, Q, k = 3000, 48, 10
    V = rng.standard_normal((N, d)).astype(np.float32)
    ck = rng.integers(0, 12, size=N).astype(np.int32) * 5 - 20
    ck[:300] = 100                                                  # one bucket of two segments
    ids = (rng.permutation(N) * 3 - 1000).astype(np.int32)
    q = dev(rng.standard_normal((Q, d)).astype(np.float32))
    tab = np.stack([rng.permutation(np.r_[np.arange(12) * 5 - 20, 100])[:4] for _ in range(Q)]).astype(np.int32)
    keys, nkeys = dev(tab), dev(rng.integers(0, 5, size=Q).astype(np.int32))
    local = rng.random(N) < 0.4
    for metric in ("l2", "cosine"):
        mk = lambda sel: Indexer(_hasher(d), dev(V[sel]), _dist(metric), algo="tiled", compat=False, row_ids=dev(ids[sel]),      # noqa: E731
                                 corpus_keys=dev(ck[sel]))
        ix = mk(slice(None))
        F = ix.row_filter(mask=dev(np.isin(np.arange(int(ids.max()) + 1), ids[local])))     # ids >= 0 by the mask, negative ones denied ...
        twin = mk(local & (ids >= 0))                                                    # ... so the twin holds the non-negative allowed ids
        got = ix.scan_tensors(q, keys, nkeys, k=k, want_keys=True, filter=F)
        _raw_equal(got, twin.scan_tensors(q, keys, nkeys, k=k, want_keys=True), (d, metric))
        _same(got[2], ix.scan_tensors(q, keys, nkeys, k=k)[2], (d, metric, "ncand"))


# ---------------------------------------------------------------------------------------------- facade
def _facade_world(N=6000, d=32, Q=300, seed=4, ids=None):
    from nlsh_amd.indexer import Indexer
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((N, d)).astype(np.float32)
    hashing = _hasher(d)
    ids = (np.arange(N) * 3 + 11).astype(np.int32) if ids is None else ids
    ix = Indexer(hashing, dev(V), _dist("l2"), compat=False, row_ids=dev(ids))
    pick = rng.choice(N, size=Q, replace=False)
    q = dev(V[pick] + 0.05 * rng.standard_normal((Q, d)).astype(np.float32))
    return rng, V, ids, hashing, ix, q


def _twin_of(ix, hashing, V, ids, local):
    from nlsh_amd.indexer import Indexer
    return Indexer(hashing, dev(V[local]), _dist("l2"), compat=False, algo="tiled", row_ids=dev(ids[local]),
                   corpus_keys=ix.corpus_keys[dev(np.flatnonzero(local))].contiguous())


def test_query_with_a_filter_equals_the_twins_lists():
    rng, V, ids, hashing, ix, q = _facade_world()
    k = 10
    local = rng.random(len(ids)) < 0.3
    # by construction for the first call below (hash_times=10, seed=5): every third query keeps at most two of its candidates, every
    # third none -- a query's candidates are the rows whose bucket key is among its keys
    keys, nkeys = ix.hash_device(q, hash_times=10, seed=5)
    kh, nh, ck = keys.cpu().numpy(), nkeys.cpu().numpy(), ix.corpus_keys.cpu().numpy()
    cands = [np.flatnonzero(np.isin(ck, kh[qi, :nh[qi]])) for qi in range(len(nh))]
    for qi in range(1, len(nh), 3):
        local[cands[qi]] = False
        local[cands[qi][:2]] = True
    for qi in range(0, len(nh), 3):
        local[cands[qi]] = False
    F = ix.row_filter(allow=ids[local].tolist())
    twin = _twin_of(ix, hashing, V, ids, local)
    seen = set()
    for kw in (dict(hash_times=10, seed=5), dict(hash_times=12, probes="ranked"), dict(hash_times=100, seed=6), dict(hash_times=1, seed=7)):
        lists, ncand = ix.query(q, k=k, filter=F, **kw)
        assert ix.last_query_path == "two_step" and ix.last_algo == _capi.SCAN_BUCKET_TILED
        want, want_nc = twin.query(q, k=k, **kw)
        assert lists == want, kw
        assert ncand == ix.query(q, k=k, **kw)[1], "candidate counts are the unfiltered call's"
        allowed = set(ids[local].tolist())
        assert all(set(row) <= allowed and len(row) == min(k, nc) for row, nc in zip(lists, want_nc))
        seen |= {"full" if len(r) == k else ("empty" if not r else "short") for r in lists}
        # the device-resident form and the caller-supplied keys form
        d_, i_, nc_, k64 = ix.query_tensors(q, k=k, want_keys=True, filter=F, **kw)
        assert ix.last_query_path == "two_step"
        t_ = twin.query_tensors(q, k=k, want_keys=True, **kw)
        _raw_equal((d_, i_, nc_, k64), t_, kw)
        if kw == dict(hash_times=10, seed=5):
            assert not any(lists[qi] for qi in range(0, len(nh), 3)) and any(0 < len(lists[qi]) < k for qi in range(1, len(nh), 3))
    assert {"short", "empty"} <= seen, seen
    keys, nkeys = ix.hash_device(q, hash_times=6, seed=8)
    kh, nh = keys.cpu().numpy(), nkeys.cpu().numpy()
    key_lists = [[int(v) & 0xFFFFFFFF for v in kh[i, :nh[i]]] for i in range(len(nh))]
    res, nc, dist, idx = ix.query_with_keys(q, key_lists, k=k, filter=F)
    tres, _, tdist, tidx = twin.query_with_keys(q, key_lists, k=k)
    assert res == tres and torch.equal(idx, tidx) and torch.equal(dist.view(torch.int32), tdist.view(torch.int32))
    assert nc == ix.query_with_keys(q, key_lists, k=k)[1]


def test_query_with_a_filter_and_a_candidate_budget():
    """The budget counts bucket rows before the filter, so the twin (other bucket sizes) stops elsewhere: the reference is the same
    index's own unfiltered k = 256 result of the same budgeted call, post-filtered, on the queries of at most 256 candidates."""
    rng, V, ids, hashing, ix, q = _facade_world(seed=12)
    k, kw = 10, dict(hash_times=16, probes="ranked", candidate_budget=40)
    local = rng.random(len(ids)) < 0.5
    allowed = set(ids[local].tolist())
    F = ix.row_filter(deny=dev(ids[~local]))
    lists, ncand = ix.query(q, k=k, filter=F, **kw)
    assert ix.last_query_path == "two_step"
    _, wi, wn, wk = ix.query_tensors(q, k=256, want_keys=True, **kw)
    wi, wn, wk = wi.cpu().numpy(), wn.cpu().numpy(), wk.cpu().numpy()
    assert ncand == wn.tolist()
    small = np.flatnonzero(wn <= 256)
    assert len(small) > 0
    for qi in small.tolist():
        assert lists[qi] == [int(wi[qi, j]) for j in range(256) if wk[qi, j] != -1 and int(wi[qi, j]) in allowed][:k], qi


def test_a_row_whose_id_is_minus_one_is_returned():
    from nlsh_amd.indexer import Indexer
    rng = np.random.default_rng(2)
    N, d, k = 40, 8, 5
    V = rng.standard_normal((N, d)).astype(np.float32)
    ids = np.arange(N, dtype=np.int32) - 18                       # row 17 has id -1
    ix = Indexer(_hasher(d), dev(V), _dist("l2"), compat=False, row_ids=dev(ids), corpus_keys=dev(np.full(N, 5, np.int32)))
    q = dev(V[[17, 3]])
    res, nc, _, _ = ix.query_with_keys(q, [[5], [5]], k=k, filter=ix.row_filter(deny=[-15]))
    assert res[0][0] == -1 and len(res[0]) == k and -15 not in res[0] + res[1] and nc == [N, N]
    res, _, _, idx = ix.query_with_keys(q, [[5], [5]], k=k, filter=ix.row_filter(allow=[-1]))
    assert res == [[-1], [-1]] and idx.cpu().tolist() == [[-1] * k] * 2


# ---------------------------------------------------------------------------------------------- staleness and refusals
def _twin_of_sorted(ix, allowed_ids):
    """The twin of a (mutated) index, from the index's own rows: its sorted rows, their ids and their bucket keys."""
    from nlsh_amd.indexer import Indexer
    keep = torch.isin(ix.gid, allowed_ids)
    keys_sorted = torch.repeat_interleave(ix.uniq_keys, torch.diff(ix.offsets).long())
    return Indexer(ix._hashing, ix.corpus_sorted[keep][:, :ix.dim].contiguous(), _dist("l2"), compat=False, algo="tiled",
                   row_ids=ix.gid[keep].contiguous(), corpus_keys=keys_sorted[keep].contiguous())


def test_stale_and_foreign_filters_raise_and_a_rebuilt_filter_equals_the_twin():
    rng, V, ids, hashing, ix, q = _facade_world(N=3000, Q=100, seed=21)
    other = _facade_world(N=3000, Q=100, seed=21)[4]
    k, kw = 10, dict(hash_times=8, seed=3)
    keys, nkeys = ix.hash_device(q, **kw)
    allow = dev(ids[rng.random(len(ids)) < 0.5])
    F = ix.row_filter(allow=allow)
    ix.query(q, k=k, filter=F, **kw)
    with pytest.raises(ValueError, match="another index"):
        other.query(q, k=k, filter=F, **kw)
    with pytest.raises(ValueError, match="another index"):
        other.scan_tensors(q, keys, nkeys, k=k, filter=F)
    forced = _facade_world(N=500, Q=10, seed=22)[4]
    forced.algo = "query"
    with pytest.raises(ValueError, match="tiled"):
        forced.query(q[:10], k=k, filter=forced.row_filter(allow=[11]), **kw)
    assert ix.remove([int(ids[0]) + 1]) == 0 and ix.query(q, k=k, filter=F, **kw) is not None     # an ineffective removal changes nothing
    new = dev(rng.standard_normal((200, V.shape[1])).astype(np.float32))
    new_ids = ix.add(new, ids=dev(np.arange(200, dtype=np.int32) - 500))
    for call in (lambda: ix.query(q, k=k, filter=F, **kw), lambda: ix.query_tensors(q, k=k, filter=F, **kw),
                 lambda: ix.scan_tensors(q, keys, nkeys, k=k, filter=F)):
        with pytest.raises(ValueError, match="stale"):
            call()
    allow2 = torch.cat([allow, new_ids[::2]])
    F2 = ix.row_filter(allow=allow2)
    _raw_equal(ix.scan_tensors(q, keys, nkeys, k=k, want_keys=True, filter=F2),
               _twin_of_sorted(ix, allow2).scan_tensors(q, keys, nkeys, k=k, want_keys=True), "after add")
    assert ix.remove(allow2[:300]) == 300
    with pytest.raises(ValueError, match="stale"):
        ix.scan_tensors(q, keys, nkeys, k=k, filter=F2)
    F3 = ix.row_filter(allow=allow2)                                # the removed ids are unknown now, and ignored
    assert F3.n_allowed == F2.n_allowed - 300
    _raw_equal(ix.scan_tensors(q, keys, nkeys, k=k, want_keys=True, filter=F3),
               _twin_of_sorted(ix, allow2).scan_tensors(q, keys, nkeys, k=k, want_keys=True), "after remove")


# ---------------------------------------------------------------------------------------------- C ABI
def test_the_filtered_call_with_a_null_filter_is_the_typed_call():
    from nlsh_amd.indexer import _SCAN_ARGS_AFTER_QUERIES, _SCAN_ARGS_BEFORE_QUERIES, _STORAGES
    L, k = _capi.lib(), 10
    for storage, kind in (("float32", "float16"), ("float16", "float16"), ("uint8", "uint8")):
        w = _world(kind)
        for algo, code in (("query", _capi.SCAN_QUERY_MAJOR), ("bucket", _capi.SCAN_BUCKET_MAJOR), ("tiled", _capi.SCAN_BUCKET_TILED)):
            if storage != "float32" and algo != "tiled":
                continue
            ix = _index(w, storage, "l2")
            ix.algo = algo
            q, keys, nkeys = w["q"], w["keys"], w["nkeys"]
            want = ix.scan_tensors(q, keys, nkeys, k=k, want_keys=True)
            max_tasks, window = ix._last_max_tasks, ix.last_window
            out_dist, pack, out_idx, ncand, status, out_keys = ix._outputs(w["Q"], k, q.device, True)
            ws = torch.zeros((L.nlsh_scan_workspace(w["Q"], w["P"], k, max_tasks, ix.n_buckets, SD),), dtype=torch.uint8, device=q.device)
            f = ix._scan_fields(w["Q"], SD, keys, nkeys, k, code, max_tasks, out_dist, out_idx, out_keys, ncand, status, ws, window)
            before = _SCAN_ARGS_BEFORE_QUERIES(f)
            _capi.check(L.nlsh_scan_topk_cells_phase_filtered(before[0], _STORAGES[storage][1], *before[1:], q.data_ptr(), q.stride(0),
                                                              *_SCAN_ARGS_AFTER_QUERIES(f), None, None, torch.cuda.current_stream().cuda_stream,
                                                              _capi.PHASE_ALL, None))
            _raw_equal((out_dist, out_idx, ncand, out_keys), want, (storage, algo))
            _same(ncand, want[2], (storage, algo, "ncand"))
            assert status.cpu().tolist()[1] == 0
