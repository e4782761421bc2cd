"""Per-query tag filters against THEIR DEFINITION: query q of a tagged call gets, word for word, what the same call gives
on the index built from the rows that pass q's mask alone -- ids, distance bits and the 64-bit sort keys, padding included -- while the
candidate counts stay the untagged call's.  The references are the existing row-filter path (one `filter=` call per distinct mask, the
rows of the queries that carry it compared), the constructor on the passing rows (`row_ids=`, `corpus_keys=`) and the CPU oracle, never
the code under test; every comparison is `torch.equal` on raw bits.  The pass rule, the masks and the tags are tests/row_tags_ref.py's,
whose coverage of full, short and empty lists tests/test_row_tags_cpu.py holds."""
import numpy as np
import pytest
import torch

import row_tags_ref as ref
from helpers import dev
from nlsh_amd import _capi
from test_gpu_corpus_storage import _dist, _hasher, _same
from test_gpu_row_filter import (KS, SD, WINDOWS, _assert_padding, _assert_task_shapes, _oracle_lists, _raw_equal, _scan, _world)

pytestmark = pytest.mark.gpu

TORCH = {"float32": torch.float32, "float16": torch.float16, "uint8": torch.uint8, "sq8": torch.float32}
U64 = np.uint64


def _tag_index(w, storage, form, tags, local=None, **kw):
    """The index of the world's rows `local` (all by default) in `storage`, built by the constructor; `tags` (uint64 over ALL rows, or
    None) go in for the same rows."""
    from nlsh_amd.indexer import Indexer
    sel = slice(None) if local is None else local
    rows = dev(w["S"][sel]).to(TORCH[storage])
    if form == "folded":
        kw["l2_form"] = "folded"
    if tags is not None:
        kw["tags"] = dev(ref.as_i64(tags[sel]))
    return Indexer(_hasher(SD), rows, _dist("cosine" if form == "cosine" else "l2"), storage=storage, algo="tiled", compat=False,
                   row_ids=dev(w["ids"][sel]), corpus_keys=dev(w["corpus_keys"][sel]), **kw)


def _forced(w):
    return w["rows_of"][ref.forced_bucket(w["buckets"])]


def _group_rows(Q, j):
    return dev(np.flatnonzero(np.arange(Q) % len(ref.MASKS) == j))


def _same_rows(got, want, rows, what):
    for t, name in ((0, "dist"), (1, "idx"), (3, "keys64")):
        _same(got[t][rows], want[t][rows], (what, name))


def _allow(ix, w, local):
    return ix.row_filter(allow=dev(w["ids"][local]))


# ---------------------------------------------------------------------------------------------- 1. the definition, through the filter path
@pytest.mark.parametrize("storage", ["float32", "float16", "uint8", "sq8"])
@pytest.mark.parametrize("form", ["l2", "folded", "cosine"])
def test_tagged_scan_equals_the_filtered_scan_of_every_mask(form, storage):
    w = _world("uint8" if storage == "uint8" else "float16")
    N, Q = len(w["ids"]), w["Q"]
    masks = ref.query_masks(Q)
    masks_d = dev(ref.as_i64(masks))
    groups = [_group_rows(Q, j) for j in range(len(ref.MASKS))]
    for mode in ref.MODES:
        tags = ref.tags_for(mode, N, _forced(w))
        ix = _tag_index(w, storage, form, tags)
        assert torch.equal(ix.tags_sorted, dev(ref.as_i64(tags))[ix.perm.long()])
        if mode == ref.MODES[0]:
            ix.window_rows = 0
            _scan(ix, w, 10, tag_mask=masks_d, tag_match=mode)
            _assert_task_shapes(ix, w)         # every (queries per wave) x (1..4 tiles) body, the single-stage body, two groups per bucket
        filters = [_allow(ix, w, ref.passes(tags, m, mode)) for m in ref.MASKS]
        for window in WINDOWS:
            ix.window_rows = window
            for k in KS:
                what = (form, storage, mode, window, k)
                plain = _scan(ix, w, k)
                got = _scan(ix, w, k, tag_mask=masks_d, tag_match=mode)
                assert ix.last_window == window and ix.last_algo == _capi.SCAN_BUCKET_TILED
                _same(got[2], plain[2], (what, "ncand is the untagged call's"))
                for j, F in enumerate(filters):
                    _same_rows(got, _scan(ix, w, k, filter=F), groups[j], (what, "mask", j))
                if (mode, 0) in ref.EMPTY_GROUPS or (mode, 6) in ref.EMPTY_GROUPS:
                    j = 0 if mode == "any" else 6
                    _assert_padding(tuple(None if t is None else t[groups[j]] for t in got), (what, "nothing passes"))


# ---------------------------------------------------------------------------------------------- 2. second angle: the constructor, the oracle
@pytest.mark.parametrize("storage", ["float32", "float16"])
def test_tagged_scan_equals_the_index_built_from_the_passing_rows(storage):
    w = _world("float16")
    N = len(w["ids"])
    for mode, mask in (("any", ref.HALVES), ("all", ref.THREE)):
        tags = ref.tags_bits(N, _forced(w))
        local = ref.passes(tags, mask, mode)
        assert 0.05 * N < local.sum() < 0.95 * N
        ix = _tag_index(w, storage, "l2", tags)
        twin = _tag_index(w, storage, "l2", None, local)
        for window in (0, 128):
            ix.window_rows = twin.window_rows = window
            for k in (10, 100):
                # one Python int for the whole batch (bit 62 among THREE's: the unsigned value goes in as it is)
                got = _scan(ix, w, k, tag_mask=int(mask), tag_match=mode)
                _raw_equal(got, _scan(twin, w, k), (storage, mode, window, k))
                _same(got[2], _scan(ix, w, k)[2], "ncand")
                if storage == "float32" and k == 10:
                    od, oi = _oracle_lists(w, local, 10)
                    assert np.array_equal(got[1].cpu().numpy(), oi), (mode, window)
                    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), od.view(np.uint32)), (mode, window)


# ---------------------------------------------------------------------------------------------- 3. tags AND a RowFilter
@pytest.mark.parametrize("storage", ["float32", "sq8"])
def test_tags_and_a_row_filter_equal_the_filter_of_the_conjunction(storage):
    w = _world("float16")
    N, Q = len(w["ids"]), w["Q"]
    masks_d = dev(ref.as_i64(ref.query_masks(Q)))
    half = np.random.default_rng(8).random(N) < 0.5
    for mode in ref.MODES:
        tags = ref.tags_for(mode, N, _forced(w))
        ix = _tag_index(w, storage, "l2", tags)
        F = _allow(ix, w, half)
        both = [_allow(ix, w, half & ref.passes(tags, m, mode)) for m in ref.MASKS]
        for window in (0, 64):
            ix.window_rows = window
            for k in (10, 100):
                got = _scan(ix, w, k, filter=F, tag_mask=masks_d, tag_match=mode)
                _same(got[2], _scan(ix, w, k)[2], "ncand")
                for j, Fj in enumerate(both):
                    _same_rows(got, _scan(ix, w, k, filter=Fj), _group_rows(Q, j), (storage, mode, window, k, j))


# ---------------------------------------------------------------------------------------------- 4. degenerate masks, the C entries without tags
@pytest.mark.parametrize("storage", ["float32", "float16", "uint8", "sq8"])
def test_all_pass_is_the_untagged_call_and_none_pass_is_padding(storage):
    w = _world("uint8" if storage == "uint8" else "float16")
    tags = ref.tags_bits(len(w["ids"]), _forced(w))
    for form in ("l2", "cosine"):
        ix = _tag_index(w, storage, form, tags)
        for window in (0, 256):
            ix.window_rows = window
            for k in (10, 256):
                plain = _scan(ix, w, k)
                for mask in (0, dev(np.zeros(w["Q"], np.int64))):
                    got = _scan(ix, w, k, tag_mask=mask, tag_match="all")
                    _raw_equal(got, plain, (storage, form, window, k, "all-pass"))
                    _same(got[2], plain[2], "ncand")
                    none = _scan(ix, w, k, tag_mask=mask, tag_match="any")
                    _assert_padding(none, (storage, form, window, k, "none-pass"))
                    _same(none[2], plain[2], "ncand")


@pytest.mark.parametrize("storage", ["float32", "uint8", "sq8"])
def test_the_tagged_calls_without_tags_are_the_base_calls(storage):
    from nlsh_amd.indexer import _SCAN_ARGS_AFTER_QUERIES, _SCAN_ARGS_BEFORE_QUERIES, _STORAGES
    L, k = _capi.lib(), 10
    w = _world("uint8" if storage == "uint8" else "float16")
    ix = _tag_index(w, storage, "l2", None)
    q, keys, nkeys = w["q"], w["keys"], w["nkeys"]
    local = np.random.default_rng(4).random(len(w["ids"])) < 0.5
    for F in (None, _allow(ix, w, local)):
        want = ix.scan_tensors(q, keys, nkeys, k=k, want_keys=True, filter=F)
        max_tasks, window = ix._last_max_tasks, ix.last_window
        out_dist, pack, out_idx, ncand, status, out_keys = ix._outputs(w["Q"], k, q.device, True)
        ws = torch.zeros((L.nlsh_scan_workspace(w["Q"], w["P"], k, max_tasks, ix.n_buckets, SD),), dtype=torch.uint8, device=q.device)
        f = ix._scan_fields(w["Q"], SD, keys, nkeys, k, _capi.SCAN_BUCKET_TILED, max_tasks, out_dist, out_idx, out_keys, ncand, status, ws, window)
        before = _SCAN_ARGS_BEFORE_QUERIES(f)
        call, store = ((L.nlsh_scan_topk_cells_phase_sq8_tagged, (ix._qlo.data_ptr(), ix._qstep.data_ptr())) if storage == "sq8"
                       else (L.nlsh_scan_topk_cells_phase_tagged, (_STORAGES[storage][1],)))
        _capi.check(call(before[0], *store, *before[1:], q.data_ptr(), q.stride(0), *_SCAN_ARGS_AFTER_QUERIES(f), None, None,
                         torch.cuda.current_stream().cuda_stream, _capi.PHASE_ALL, None if F is None else F.words.data_ptr(), None, None, 99))
        _raw_equal((out_dist, out_idx, ncand, out_keys), want, (storage, F is not None))
        _same(ncand, want[2], "ncand")
        assert status.cpu().tolist()[1] == 0


# ---------------------------------------------------------------------------------------------- 5. denied rows cannot poison a list
@pytest.mark.parametrize("storage", ["float32", "float16"])
@pytest.mark.parametrize("form", ["l2", "cosine"])
def test_denied_non_finite_rows_change_nothing(form, storage):
    base = _world("float16")
    w = dict(base, S=base["S"].copy())
    rng = np.random.default_rng(9)
    N = len(w["ids"])
    bad = rng.choice(N, size=N // 8, replace=False)
    vals = np.asarray([np.nan, np.inf, -np.inf], dtype=np.float16)
    w["S"][bad, rng.integers(0, SD, size=len(bad))] = vals[rng.integers(0, 3, size=len(bad))]
    w["S"][bad[:40]] = np.float16(np.nan)
    tags = np.full(N, ref.BIT63 | U64(1), dtype=U64)
    tags[bad] = U64(1)                                              # fails ("all", bit 63 | bit 0) and ("eq", ...), passes ("any", bit 0)
    good = ~np.isin(np.arange(N), bad)
    ix = _tag_index(w, storage, form, tags)
    twin = _tag_index(w, storage, form, None, good)
    for window in (0, 64, 256):
        ix.window_rows = twin.window_rows = window
        for k in (10, 100):
            want = _scan(twin, w, k)
            for mode, mask in (("all", ref.BIT63 | U64(1)), ("eq", ref.BIT63 | U64(1)), ("any", ref.BIT63)):
                got = _scan(ix, w, k, tag_mask=int(mask), tag_match=mode)
                _raw_equal(got, want, (form, storage, window, k, mode))
                assert bool((torch.isfinite(got[0]) | (got[1] == -1)).all()), "a denied non-finite row reached a list"


# ---------------------------------------------------------------------------------------------- 6. ties
def test_the_ties_bucket_with_three_rows_passing_keeps_the_order():
    w = _world("float16")
    N = len(w["ids"])
    ties_rows = w["rows_of"][w["ties"]]
    tags = np.full(N, U64(1 << 40), dtype=U64)
    tags[np.setdiff1d(ties_rows, ties_rows[[3, 100, 255]])] = U64(1 << 39)
    local = tags == U64(1 << 40)
    ix = _tag_index(w, "float32", "l2", tags)
    twin = _tag_index(w, "float32", "l2", None, local)
    denied = set(w["ids"][np.setdiff1d(ties_rows, ties_rows[[3, 100, 255]])].tolist())
    for window in (0, 256):
        ix.window_rows = twin.window_rows = window
        for k in (1, 10, 100):
            got = _scan(ix, w, k, tag_mask=1 << 40, tag_match="any")
            _raw_equal(got, _scan(twin, w, k), (window, k))
            dist, idx = got[0].cpu().numpy(), got[1].cpu().numpy()
            assert not (set(idx.reshape(-1).tolist()) & denied)
            for row_d, row_i in zip(dist, idx):
                same = (row_d[1:] == row_d[:-1]) & np.isfinite(row_d[1:])
                row_u = row_i.view(np.uint32)                       # the sort key's id word: ties in unsigned id order
                assert np.all(row_u[1:][same] > row_u[:-1][same])


# ---------------------------------------------------------------------------------------------- 7. mutations
def _rand64(rng, n):
    return (rng.integers(0, 1 << 32, size=n, dtype=np.uint64) << U64(32)) | rng.integers(0, 1 << 32, size=n, dtype=np.uint64)


class _Mirror:
    """The index's rows in LOCAL order on the host: the constructor's, then every added batch, minus the removed rows."""

    def __init__(self, d, n, rng):
        self.d, self.rng = d, rng
        self.V = rng.standard_normal((n, d)).astype(np.float32)
        self.ids = (np.arange(n) * 2 - 301).astype(np.int32)
        self.keys = (rng.integers(0, 9, size=n) * 7 - 20).astype(np.int32)
        self.tags = self.draw_tags(n)
        self.next = int(self.ids.max()) + 5

    def draw_tags(self, n):
        return _rand64(self.rng, n) & _rand64(self.rng, n)          # a quarter of the 64 bits, bit 63 among them

    def build(self, with_tags=True):
        from nlsh_amd.indexer import Indexer
        kw = dict(tags=dev(ref.as_i64(self.tags))) if with_tags else {}
        return Indexer(_hasher(self.d), dev(self.V), _dist("l2"), algo="tiled", compat=False, row_ids=dev(self.ids),
                       corpus_keys=dev(self.keys), **kw)

    def new_rows(self, m):
        V = self.rng.standard_normal((m, self.d)).astype(np.float32)
        ids = (self.next + np.arange(m) * 3).astype(np.int32)
        self.next = int(ids.max()) + 1 if m else self.next
        keys = (self.rng.integers(0, 11, size=m) * 7 - 20).astype(np.int32)
        return V, ids, keys, self.draw_tags(m)

    def apply(self, remove=None, add=None, default_tags=False):
        if remove is not None:
            keep = ~np.isin(self.ids, remove)
            self.V, self.ids, self.keys, self.tags = self.V[keep], self.ids[keep], self.keys[keep], self.tags[keep]
        if add is not None:
            V, ids, keys, tags = add
            tags = np.zeros(len(ids), U64) if default_tags else tags
            self.V, self.ids, self.keys, self.tags = np.r_[self.V, V], np.r_[self.ids, ids], np.r_[self.keys, keys], np.r_[self.tags, tags]


def _assert_is_the_rebuild(ix, m, q, keys, nkeys, what):
    assert torch.equal(ix.tags_sorted, dev(ref.as_i64(m.tags))[ix.perm.long()]), (what, "tags_sorted == tags[perm]")
    assert torch.equal(ix.tags_local(), dev(ref.as_i64(m.tags))), what
    rebuilt = m.build()
    assert torch.equal(ix.gid, rebuilt.gid) and torch.equal(ix.tags_sorted, rebuilt.tags_sorted), what
    masks = dev(ref.as_i64(_rand64(m.rng, q.shape[0]) & _rand64(m.rng, q.shape[0]) & _rand64(m.rng, q.shape[0])))
    for mode in ref.MODES:
        for mask in (masks, 1, (1 << 63) | 6):
            a = ix.scan_tensors(q, keys, nkeys, k=10, want_keys=True, tag_mask=mask, tag_match=mode)
            b = rebuilt.scan_tensors(q, keys, nkeys, k=10, want_keys=True, tag_mask=mask, tag_match=mode)
            _raw_equal(a, b, (what, mode))
            _same(a[2], b[2], (what, mode, "ncand"))


@pytest.mark.parametrize("d", [1, 100])
def test_tags_follow_the_rows_through_every_mutation(d):
    rng = np.random.default_rng(40 + d)
    m = _Mirror(d, 1500, rng)
    ix = m.build()
    Q = 40
    q = dev(rng.standard_normal((Q, d)).astype(np.float32))
    tab = np.stack([rng.permutation(np.arange(11) * 7 - 20)[:4] for _ in range(Q)]).astype(np.int32)
    keys, nkeys = dev(tab), dev(rng.integers(1, 5, size=Q).astype(np.int32))
    _assert_is_the_rebuild(ix, m, q, keys, nkeys, "built")
    gen = ix.generation
    # add(tags=)
    new = m.new_rows(300)
    ix.add(dev(new[0]), ids=dev(new[1]), keys=dev(new[2]), tags=dev(ref.as_i64(new[3])))
    m.apply(add=new)
    _assert_is_the_rebuild(ix, m, q, keys, nkeys, "add")
    # remove
    gone = rng.choice(m.ids, size=400, replace=False)
    assert ix.remove(dev(gone)) == 400
    m.apply(remove=gone)
    _assert_is_the_rebuild(ix, m, q, keys, nkeys, "remove")
    # both in one update
    gone, new = rng.choice(m.ids, size=250, replace=False), m.new_rows(120)
    ix.update(add=dev(new[0]), add_ids=dev(new[1]), add_keys=dev(new[2]), add_tags=dev(ref.as_i64(new[3])), remove=dev(gone))
    m.apply(remove=gone, add=new)
    _assert_is_the_rebuild(ix, m, q, keys, nkeys, "update")
    assert ix.generation == gen + 3
    # set_tags: in place, no row moves, the generation stays, unknown ids are ignored
    F = ix.row_filter(allow=dev(m.ids[::2]))
    pick = rng.choice(len(m.ids), size=200, replace=False)
    fresh = m.draw_tags(200)
    unknown = np.asarray([int(m.ids.max()) + 1000, -(1 << 30)], dtype=np.int32)
    found = ix.set_tags(dev(np.r_[m.ids[pick], unknown]), dev(ref.as_i64(np.r_[fresh, np.zeros(2, U64)])))
    assert found == 200 and ix.generation == gen + 3
    m.tags[pick] = fresh
    _assert_is_the_rebuild(ix, m, q, keys, nkeys, "set_tags")
    ix.scan_tensors(q, keys, nkeys, k=10, filter=F, tag_mask=1)        # a RowFilter built before set_tags is not stale
    # the default tag, and an emptied index
    new = m.new_rows(50)
    ix.add(dev(new[0]), ids=dev(new[1]), keys=dev(new[2]))
    m.apply(add=new, default_tags=True)
    assert int((ix.tags_sorted == 0).sum()) >= 50
    _assert_is_the_rebuild(ix, m, q, keys, nkeys, "default tag 0")
    assert ix.remove(dev(m.ids)) == len(m.ids)
    assert ix.tags_sorted.numel() == 0
    _assert_padding(ix.scan_tensors(q, keys, nkeys, k=10, want_keys=True, tag_mask=0, tag_match="all"), "emptied")
    m.apply(remove=m.ids)
    new = m.new_rows(64)
    ix.add(dev(new[0]), ids=dev(new[1]), keys=dev(new[2]), tags=dev(ref.as_i64(new[3])))
    m.apply(add=new)
    _assert_is_the_rebuild(ix, m, q, keys, nkeys, "refilled")
    with pytest.raises(ValueError, match="built without tags"):
        m.build(with_tags=False).add(dev(new[0]), ids=dev(new[1] + 9999), keys=dev(new[2]), tags=dev(ref.as_i64(new[3])))


# ---------------------------------------------------------------------------------------------- 8. facade and composition
def _facade(N=6000, d=32, Q=294, seed=4, mode="any", **kw):
    from nlsh_amd.indexer import Indexer
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((N, d)).astype(np.float32)
    tags = ref.tags_for(mode, N, np.arange(2 * ref.N_FORCED))
    ix = Indexer(_hasher(d), dev(V), _dist("l2"), compat=False, tags=dev(ref.as_i64(tags)), **kw)
    pick = rng.choice(N, size=Q, replace=False)
    q = dev(V[pick] + 0.05 * rng.standard_normal((Q, d)).astype(np.float32))
    ids = np.arange(N, dtype=np.int64) + ix.id_base
    return V, tags, ids, ix, q


def test_query_forms_equal_the_filtered_calls_of_every_mask():
    k = 10
    for mode in ref.MODES:
        V, tags, ids, ix, q = _facade(mode=mode)
        Q = q.shape[0]
        masks_d = dev(ref.as_i64(ref.query_masks(Q)))
        filters = [ix.row_filter(allow=dev(ids[ref.passes(tags, m, mode)])) for m in ref.MASKS]
        lengths = set()
        for kw in (dict(hash_times=10, seed=5), dict(hash_times=12, probes="ranked"), dict(hash_times=16, probes="ranked", candidate_budget=40),
                   dict(hash_times=70, seed=6), dict(hash_times=1, seed=7)):
            lists, ncand = ix.query(q, k=k, tag_mask=masks_d, tag_match=mode, **kw)
            assert ix.last_query_path == "two_step" and ix.last_algo == _capi.SCAN_BUCKET_TILED
            got = ix.query_tensors(q, k=k, want_keys=True, tag_mask=masks_d, tag_match=mode, **kw)
            assert ix.last_query_path == "two_step"
            lens = (got[3] != -1).sum(dim=1).cpu().tolist()
            assert [len(row) for row in lists] == lens, "list lengths come from the sort keys"
            assert lists == [row[:n] for row, n in zip(got[1].cpu().tolist(), lens)]
            assert ncand == ix.query(q, k=k, **kw)[1], "candidate counts are the untagged call's"
            assert ncand == got[2].cpu().tolist()
            for j, F in enumerate(filters):
                rows = _group_rows(Q, j)
                want = ix.query_tensors(q, k=k, want_keys=True, filter=F, **kw)
                _same_rows(got, want, rows, (mode, kw, j))
                _same(got[2], want[2], (mode, kw, "ncand"))
                want_lists = ix.query(q, k=k, filter=F, **kw)[0]
                assert [lists[i] for i in rows.cpu().tolist()] == [want_lists[i] for i in rows.cpu().tolist()], (mode, kw, j)
            lengths |= {"full" if n == k else ("empty" if n == 0 else "short") for n in lens}
        assert "empty" in lengths and len(lengths) >= 2, lengths
        keys, nkeys = ix.hash_device(q, hash_times=6, seed=8)
        kh, nh = keys.cpu().numpy(), nkeys.cpu().numpy()
        key_lists = [[int(v) & 0xFFFFFFFF for v in kh[i, :nh[i]]] for i in range(len(nh))]
        res, nc, dist, idx = ix.query_with_keys(q, key_lists, k=k, tag_mask=masks_d, tag_match=mode)
        for j, F in enumerate(filters):
            rows = _group_rows(Q, j)
            wres, wnc, wdist, widx = ix.query_with_keys(q, key_lists, k=k, filter=F)
            assert [res[i] for i in rows.cpu().tolist()] == [wres[i] for i in rows.cpu().tolist()] and nc == wnc
            _same(dist[rows], wdist[rows], "dist")
            _same(idx[rows], widx[rows], "idx")


def test_refine_on_an_sq8_index_reranks_the_tagged_stage_one():
    V, tags, ids, ix, q = _facade(N=4000, Q=140, seed=14, mode="any", storage="sq8", refine="device")
    Q = q.shape[0]
    masks_d = dev(ref.as_i64(ref.query_masks(Q)))
    kw = dict(k=10, hash_times=8, seed=3, want_keys=True)
    got = ix.query_tensors(q, tag_mask=masks_d, tag_match="any", **kw)
    assert ix.last_query_path == "two_step+refine"
    for j, m in enumerate(ref.MASKS):
        F = ix.row_filter(allow=dev(ids[ref.passes(tags, m, "any")]))
        want = ix.query_tensors(q, filter=F, **kw)
        _same_rows(got, want, _group_rows(Q, j), ("refine", j))
        _same(got[2], want[2], "ncand")


def test_multi_table_forwards_tags_and_masks():
    from nlsh_amd.multitable import MultiTableIndexer
    rng = np.random.default_rng(31)
    N, d, Q, k = 5000, 32, 140, 10
    V = rng.standard_normal((N, d)).astype(np.float32)
    tags = ref.tags_bits(N, np.arange(2 * ref.N_FORCED))
    mt = MultiTableIndexer([_hasher(d), _hasher(d, H=12)], dev(V), _dist("l2"), tags=dev(ref.as_i64(tags)))
    assert all(torch.equal(t.tags_sorted, dev(ref.as_i64(tags))[t.perm.long()]) for t in mt.tables)
    q = dev(V[rng.choice(N, size=Q, replace=False)] + 0.05 * rng.standard_normal((Q, d)).astype(np.float32))
    masks_d = dev(ref.as_i64(ref.query_masks(Q)))
    ids = np.arange(N, dtype=np.int64)
    for mode in ("any", "all"):
        kw = dict(k=k, hash_times=6, seed=2)
        got = mt.query_tensors(q, want_keys=True, tag_mask=masks_d, tag_match=mode, **kw)
        lists = mt.query(q, tag_mask=masks_d, tag_match=mode, **kw)[0]
        for j, m in enumerate(ref.MASKS):
            rows = _group_rows(Q, j)
            F = mt.row_filter(allow=dev(ids[ref.passes(tags, m, mode)]))
            want = mt.query_tensors(q, want_keys=True, filter=F, **kw)
            _same_rows(got, want, rows, ("multi", mode, j))
            _same(got[2], want[2], "ncand")
            want_lists = mt.query(q, filter=F, **kw)[0]
            assert [lists[i] for i in rows.cpu().tolist()] == [want_lists[i] for i in rows.cpu().tolist()]
    # mutations reach every table
    new = dev(rng.standard_normal((40, d)).astype(np.float32))
    new_tags = ref.tags_bits(40, np.arange(2 * ref.N_FORCED), seed=9)
    new_ids = mt.add(new, tags=dev(ref.as_i64(new_tags)))
    assert mt.set_tags(new_ids[:3], dev(np.asarray([7, 7, 7], np.int64))) == 3
    new_tags[:3] = U64(7)
    all_tags = dev(ref.as_i64(np.r_[tags, new_tags]))
    assert all(torch.equal(t.tags_local(), all_tags) for t in mt.tables)
