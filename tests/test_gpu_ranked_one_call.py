"""The ranked multi-probe mode as one fused batch call (`nlsh_query_batch_ranked`, probe_ranked_plan_kernel) on the GPU.

The reference of every equality is the TWO-STEP path of the same indexer (`Indexer.ranked_one_call = False`: the one-probe encode,
`nlsh_probe_ranked[_budget]`, then `scan_tensors` with the stand-alone lookup), which tests/test_gpu_probe_ranked*.py pin against the
numpy references; one case here holds the one-call key table against those references directly.  Nothing has a tolerance: every word
of the key table (the zero padding included), the key counts, distance bits, ids and candidate counts are compared."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import ranked_budget_ref as rbr
import ranked_ref as rr
from helpers import dev, make_hashing

pytestmark = pytest.mark.gpu

N = 20000
BUDGETS = (None, 1, 200, 10 ** 9)


@contextlib.contextmanager
def path(one_call):
    """The class switch, for the duration of a block."""
    from nlsh_amd.indexer import Indexer
    old = Indexer.ranked_one_call
    Indexer.ranked_one_call = one_call
    try:
        yield
    finally:
        Indexer.ranked_one_call = old


@functools.lru_cache(maxsize=None)
def case(d, H, compat, metric="l2", seed=3, window_rows=None, algo=None):
    """(indexer, hasher, corpus) of one index: 20,000 standard-normal rows, a gain-3 hasher (its pre-activations spread over a few
    units, so the ranked keys of a row differ a lot from row to row)."""
    from nlsh_amd import synth
    from nlsh_amd.data import SIFT, Glove
    from nlsh_amd.indexer import Indexer
    dims = [d, 64, H]
    Ws, bs = synth.make_weights(dims, seed=seed, gain=3.0)
    h = make_hashing(d, dims[1:-1], H, Ws, bs, compat=compat)
    corpus = dev(np.random.default_rng(41).standard_normal((N, d)).astype(np.float32))
    ix = Indexer(h, corpus, SIFT.distance if metric == "l2" else Glove.distance, compat=compat, window_rows=window_rows, algo=algo)
    return ix, h, corpus


def queries(Q, d, seed=7):
    return dev(np.random.default_rng(seed).standard_normal((Q, d)).astype(np.float32))


def two_step(ix, q, P, k, budget):
    """-> (keys, nkeys, dist, idx, ncand) of the parent's path: hash, then scan."""
    with path(False):
        keys, nkeys = ix.hash_device(q, hash_times=P, probes="ranked", candidate_budget=budget)
        dist, idx, ncand, _ = ix.query_tensors(q, k=k, hash_times=P, probes="ranked", candidate_budget=budget)
        assert ix.last_query_path == "two_step"
    return keys, nkeys, dist, idx, ncand


def one_call(ix, q, P, k, budget, expect="ranked_one_call"):
    """-> the same five from the public call plus the call's own key table (written into sentinel-filled tensors: every word, the
    zero padding included, must come from the kernel)."""
    with path(True):
        dist, idx, ncand, _ = ix.query_tensors(q, k=k, hash_times=P, probes="ranked", candidate_budget=budget)
        assert ix.last_query_path == expect, (ix.last_query_path, expect)
        if expect != "ranked_one_call":
            keys, nkeys = ix.hash_device(q, hash_times=P, probes="ranked", candidate_budget=budget)
            return keys, nkeys, dist, idx, ncand
        Q = q.shape[0]
        keys = torch.full((Q, P), -7, dtype=torch.int32, device=q.device)
        nkeys = torch.full((Q,), -7, dtype=torch.int32, device=q.device)
        qq = ix._as_queries(q)
        got = ix._ranked_tensors(qq, k, P, None if budget is None else ix._candidate_budget(budget, "ranked"), False, True, None,
                                 ix.choose_algo(Q, P), ix._n_multi_rows(Q), out=(keys, nkeys))
        assert torch.equal(got[0].view(torch.int32), dist.view(torch.int32)) and torch.equal(got[1], idx) and torch.equal(got[2], ncand)
    return keys, nkeys, dist, idx, ncand


def assert_same(got, want, what):
    for name, g, w in zip(("keys", "nkeys", "dist", "idx", "ncand"), got, want):
        g, w = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (g, w))
        assert g.shape == w.shape and torch.equal(g, w), (what, name, torch.nonzero(g != w)[:4].tolist())


def compare(ix, q, P, k=10, budget=None, expect="ranked_one_call", what=None):
    h = ix._hashing
    calls, mode = repr(h._calls), h.probes
    want = two_step(ix, q, P, k, budget)
    got = one_call(ix, q, P, k, budget, expect)
    assert_same(got, want, what or (q.shape, P, k, budget))
    assert repr(h._calls) == calls and h.probes == mode      # no seed was drawn, the hasher is as it was
    return got


# ---------------------------------------------------------------------------- batch sizes: partial and exact workgroups of 16 rows
@pytest.mark.parametrize("H", [8, 14])
@pytest.mark.parametrize("Q", [1, 15, 16, 17, 257])
def test_batch_sizes_around_the_workgroup(Q, H):
    ix, h, _ = case(32, H, False)
    # one query of ten probes is below the 64 pairs from which the bucket-major schedule is chosen: the query-major stream, two steps
    compare(ix, queries(Q, 32, seed=Q), 10, expect="two_step" if Q == 1 else "ranked_one_call")


# ---------------------------------------------------------------------------- probes x budgets, both lookup regimes
def test_the_two_indexes_cover_both_lookup_regimes():
    ix8, _, _ = case(32, 8, False)
    ix14, _, _ = case(32, 14, False)
    assert 1 <= ix8.n_buckets <= 256                       # the whole key table is the coarse table: stride 1
    assert ix14.n_buckets > 1024                           # coarse table of every 2nd (4th, ...) key, the fine search in global memory
    keys, nkeys = ix14.hash_device(queries(257, 32), hash_times=64, probes="ranked")
    valid = (torch.arange(64, device=keys.device)[None, :] < nkeys[:, None])
    present = torch.isin(keys, ix14.uniq_keys)
    assert (valid & ~present).any() and (valid & present).any()      # probes with no bucket, and probes with one


@pytest.mark.parametrize("H", [8, 14])
@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("P", [1, 2, 10, 64])
def test_probes_and_budgets(P, budget, H):
    ix, h, _ = case(32, H, False)
    keys, nkeys, _, _, ncand = compare(ix, queries(257, 32), P, budget=budget)
    if budget == 200 and P >= 10 and H == 14:
        full = ix.hash_device(queries(257, 32), hash_times=P, probes="ranked")[1]
        assert (nkeys < full).any()                        # the budget does cut


def test_the_key_table_is_the_reference_table():
    """The one-call kernel's keys against tests/ranked_ref.py / ranked_budget_ref.py directly, on the encoder's own z and hard codes."""
    from nlsh_amd import _capi
    ix, h, _ = case(32, 14, False)
    q = queries(257, 32)
    z, _, code = h.forward_device(q)
    z, code = z.cpu().numpy(), code.cpu().numpy().view(np.uint32)
    uniq, offsets = ix.uniq_keys.cpu().numpy(), ix.offsets.cpu().numpy()
    full = rr.table(z, code, 14, 10, _capi.KEY_FULL)
    for budget in (None, 200):
        keys, nkeys, _, _, ncand = one_call(ix, q, 10, 10, budget)
        want = full if budget is None else rbr.cut(*full, uniq, offsets, budget)
        assert np.array_equal(keys.cpu().numpy(), want[0]) and np.array_equal(nkeys.cpu().numpy(), want[1]), budget
        if budget is not None:
            assert np.array_equal(ncand.cpu().numpy(), want[3])


# ---------------------------------------------------------------------------- int16 keys of a 20-bit hash: dead slots, the single-probe tail
def test_colliding_int16_keys_leave_dead_slots_and_the_trailing_batch_has_one_key():
    ix, h, _ = case(32, 20, True)
    Q = 4096 + 5                                           # HASH_BATCH semantics: the five rows behind the full batch are single-probe
    for budget in (None, 200):
        keys, nkeys, _, _, _ = compare(ix, queries(Q, 32), 10, budget=budget)
        assert (nkeys[4096:] == 1).all() and (keys[4096:, 1:] == 0).all()
        if budget is None:
            assert (nkeys[:4096] < 10).any() and (nkeys[:4096] == 10).any()      # some rows lost slots to a repeated 16-bit key


# ---------------------------------------------------------------------------- the tiled schedule's query copy
@pytest.mark.parametrize("d,metric", [(100, "l2"), (30, "l2"), (100, "cosine")], ids=["aligned-no-copy", "padded-copy", "normalised-copy"])
def test_query_preparation(d, metric):
    ix, h, _ = case(d, 12, False, metric=metric)
    compare(ix, queries(257, d), 10)
    compare(ix, queries(257, d), 10, budget=200)


@pytest.mark.parametrize("width", [128, 101], ids=["stride-128", "stride-101"])
def test_a_strided_view_as_queries(width):
    d = 100
    ix, h, _ = case(d, 12, False)
    wide = np.full((257, width), np.nan, dtype=np.float32)
    wide[:, :d] = queries(257, d).cpu().numpy()
    q_wide = dev(wide)
    view = q_wide[:, :d]
    assert view.stride(0) == width
    got = compare(ix, view, 10, what=("view", width))
    assert_same(got, one_call(ix, view.contiguous(), 10, 10, None), ("contiguous copy", width))


# ---------------------------------------------------------------------------- schedules and k
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("algo", ["tiled", "bucket"])
@pytest.mark.parametrize("window_rows", [0, 64])
def test_schedules_windows_and_k(window_rows, algo, k):
    from nlsh_amd import _capi
    ix, h, _ = case(32, 14, False, window_rows=window_rows, algo=algo)
    q = queries(300, 32)
    if algo == "bucket" and k > _capi.MAX_K:
        # the wave-level schedule takes k <= 64 on every path: both forms refuse the batch the same way, before a launch
        for mode in (False, True):
            with path(mode), pytest.raises(_capi.NlshHipError) as e:
                ix.query_tensors(q, k=k, hash_times=10, probes="ranked")
            assert e.value.code == _capi.E_UNSUPPORTED
        return
    compare(ix, q, 10, k=k)
    compare(ix, q, 10, k=k, budget=200)
    with path(False):
        want = ix.query(q, k=k, hash_times=10, probes="ranked")
        assert ix.last_query_path == "two_step"
    with path(True):
        got = ix.query(q, k=k, hash_times=10, probes="ranked")
        assert ix.last_query_path == "ranked_one_call"
        assert ix._host_form(k, ("ranked", 0, 300)) == (k <= 64)          # k = 100 stays on the copy form
    assert got == want


# ---------------------------------------------------------------------------- query(): ranges, the F7 fallback of short queries
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("Q,chunks", [(300, 1), (4100, 2)], ids=["one-range", "two-ranges"])
def test_query_lists_and_counts(Q, chunks, compat):
    ix, h, _ = case(32, 14, compat)
    q = queries(Q, 32, seed=Q)
    k = 10
    old = ix.query_chunks
    ix.query_chunks = chunks
    try:
        for budget in (None, 1, 200):
            with path(False):
                want = ix.query(q, k=k, hash_times=10, probes="ranked", candidate_budget=budget)
                assert ix.last_query_path == "two_step"
            with path(True):
                got = ix.query(q, k=k, hash_times=10, probes="ranked", candidate_budget=budget)
                assert ix.last_query_path == "ranked_one_call"
                again = ix.query(q, k=k, hash_times=10, probes="ranked", candidate_budget=budget)       # the kept plans, reused
            assert got[1] == want[1], budget
            assert got[0] == want[0] and again == got, budget
            if budget == 1:
                counts = np.asarray(got[1])
                assert (counts < k).any()                  # short queries: compat answers them from the key rows in the host block (F7)
                short = np.nonzero(counts < k)[0].tolist()
                assert [got[0][i] for i in short] == [want[0][i] for i in short]
        h.probes = "ranked"                                # the mode set on the hasher instead of the call
        try:
            with path(True):
                assert ix.query(q, k=k, hash_times=10) == ix.query(q, k=k, hash_times=10, probes="ranked")
                assert ix.last_query_path == "ranked_one_call"
        finally:
            h.probes = "sampled"
    finally:
        ix.query_chunks = old


# ---------------------------------------------------------------------------- task-table overflow
def test_a_task_table_overflow_is_retried_on_the_same_keys(monkeypatch):
    ref, _, _ = case(32, 14, False)
    fresh = case.__wrapped__(32, 14, False)[0]             # an indexer of its own: no task table has been sized yet
    monkeypatch.setattr(fresh, "_estimate_tasks", lambda *a, **kw: 8)
    q = queries(300, 32)
    for budget in (None, 200):
        want = two_step(ref, q, 10, 10, budget)
        fresh._max_tasks.clear()
        with path(True):
            dist, idx, ncand, _ = fresh.query_tensors(q, k=10, hash_times=10, probes="ranked", candidate_budget=budget)
            assert fresh.last_query_path == "ranked_one_call"
        assert fresh._last_max_tasks > 8 and int(fresh.last_status.cpu()[1]) == 0            # the table has grown, the batch fits
        assert_same((dist, idx, ncand), want[2:], ("overflow", budget))
        fresh._max_tasks.clear()
        fresh.__dict__.get("_range_plans", {}).clear()
        with path(False):
            lists = ref.query(q, k=10, hash_times=10, probes="ranked", candidate_budget=budget)
        with path(True):
            got = fresh.query(q, k=10, hash_times=10, probes="ranked", candidate_budget=budget)
            assert fresh.last_query_path == "ranked_one_call"
        assert fresh._last_max_tasks > 8 and got == lists


# ---------------------------------------------------------------------------- workspace contract, a sampled batch behind a ranked one
def test_the_pair_counters_are_zero_again_and_a_sampled_batch_follows():
    from nlsh_amd import _capi
    ix, h, _ = case(32, 14, False)
    q = queries(300, 32)
    one_call(ix, q, 10, 10, 200)
    stream = torch.cuda.current_stream(q.device).cuda_stream
    ws = ix._ws[(stream, True)]
    assert ix.last_algo == _capi.SCAN_BUCKET_TILED
    n_cells = ix.cells(ix.last_window)[3] if ix.last_window else ix.n_buckets
    torch.cuda.synchronize()
    assert n_cells > 0 and not ws[:4 * n_cells].any()
    dist, idx, ncand, _ = ix.query_tensors(q, k=10, hash_times=10, seed=5)
    assert ix.last_query_path == "fused"
    keys, nkeys = ix.hash_device(q, hash_times=10, seed=5)
    wdist, widx, wncand, _ = ix.scan_tensors(q, keys, nkeys, k=10)
    assert_same((dist, idx, ncand), (wdist, widx, wncand), "sampled after ranked")


# ---------------------------------------------------------------------------- weights changed in place between two calls
def test_a_weight_change_reaches_the_kept_plan():
    ix, h, _ = case.__wrapped__(32, 14, False)
    q = queries(300, 32)
    with path(True):
        before = ix.query(q, k=10, hash_times=10, probes="ranked")
    lin = [m for m in h._hasher.modules() if isinstance(m, torch.nn.Linear)][-1]
    with torch.no_grad():
        lin.weight[3].mul_(-1.0)                           # one bit of the hash flips its sign (the index keeps the old keys: only the queries move)
    with path(False):
        want = ix.query(q, k=10, hash_times=10, probes="ranked")
    with path(True):
        got = ix.query(q, k=10, hash_times=10, probes="ranked")
        assert ix.last_query_path == "ranked_one_call"
    assert got == want and got != before
