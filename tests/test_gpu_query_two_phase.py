"""`Indexer.query` builds the containers of its result while the first row range scans and stores every range's ids into its rows as
the range completes (csrc/fastlists.c `rows_alloc` / `rows_fill`).  The lists must be those of the one-shot conversion and those derived
from `query_tensors` on the same seed: for every k, split and compat mode, with short queries, across a task-table retry and under
the opt-ins."""
import gc

import numpy as np
import pytest

from helpers import dev, make_hashing
from nlsh_amd import indexer as ixmod, synth
from nlsh_amd.hashings import host_key_set

pytestmark = pytest.mark.gpu

N, D, Q = 20000, 16, 4099          # Q: two ranges of 2049 + 2050 rows, three of 1366 + 1366 + 1367
P_MAIN, SEED = 10, 20250
_cases = {}


def _case(compat, H):
    """One index per (compat, hash size) for the whole module, and the query batch on the device."""
    if "data" not in _cases:
        corpus, mean, std = synth.standardise(synth.sift_like(N, D, seed=511))
        queries = synth.standardise(synth.sift_like(Q, D, seed=512), mean, std)[0]
        _cases["data"] = dev(corpus), dev(queries)
    cg, qg = _cases["data"]
    if (compat, H) not in _cases:
        from nlsh_amd.data import SIFT
        Ws, bs = synth.make_weights([D, 32, H], seed=513)
        ix = ixmod.Indexer(make_hashing(D, [32], H, Ws, bs, compat=compat, seed=5), cg, SIFT.distance, compat=compat)
        ix._CHUNK_MIN_ROWS = 1024          # three ranges of a 4099-row batch are still ranges (the default asks 2048 rows per range)
        _cases[(compat, H)] = ix
    return _cases[(compat, H)], qg


def _derived(ix, q, k, P, seed):
    """The reference's lists from the device-resident call on the same seed: the id rows, and for a query with fewer than k candidates
    the rows of the last key of its key set (compat, F7) or its ids up to the first -1."""
    _, idx, nc, _ = ix.query_tensors(q, k=k, hash_times=P, seed=seed)
    idx, nc = idx.cpu().numpy(), nc.cpu().numpy()
    rows = idx.tolist()
    short = np.nonzero(nc < k)[0].tolist()
    if short and ix.compat:
        keys, nkeys = ix.hash_device(q, hash_times=P, seed=seed)
        keys, nkeys = keys.cpu().numpy(), nkeys.cpu().numpy()
    for qi in short:
        if ix.compat:
            order = list(host_key_set(keys[qi], int(nkeys[qi]), ix._hashing.key_mode))
            rows[qi] = ix._rows_of_key(order[-1]) if order else []
        else:
            rows[qi] = [int(v) for v in idx[qi] if v >= 0]
    return rows, nc.tolist(), len(short)


def _counting(monkeypatch):
    """Count the helper's calls: the comparison must not pass because both sides took the one-shot path."""
    calls = {"alloc": 0, "fill": 0}
    alloc, fill = ixmod._rows_alloc, ixmod._rows_fill
    assert alloc is not None and fill is not None, "csrc/fastlists.c was not built (make -C csrc)"

    def counted_alloc(*a):
        calls["alloc"] += 1
        return alloc(*a)

    def counted_fill(*a):
        calls["fill"] += 1
        return fill(*a)
    monkeypatch.setattr(ixmod, "_rows_alloc", counted_alloc)
    monkeypatch.setattr(ixmod, "_rows_fill", counted_fill)
    return calls


def _one_shot(monkeypatch, ix, *args, **kw):
    """The same call with the two-phase helper away: the one-shot conversion (`_plain_lists` per range, lists concatenated)."""
    with monkeypatch.context() as m:
        m.setattr(ixmod, "_rows_alloc", None)
        m.setattr(ixmod, "_rows_fill", None)
        return ix.query(*args, **kw)


def _plain(result):
    rows, counts = result
    assert type(rows) is list and type(counts) is list and len(rows) == len(counts)
    assert all(type(r) is list for r in rows) and all(type(c) is int for c in counts)
    assert all(type(v) is int for r in rows for v in r)
    assert gc.is_tracked(rows) and all(gc.is_tracked(r) for r in rows)
    return rows, counts


@pytest.mark.parametrize("compat", [True, False], ids=["compat", "plain"])
@pytest.mark.parametrize("chunks", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 10, 64])
def test_two_phase_query_equals_query_tensors_and_the_one_shot_path(monkeypatch, k, chunks, compat):
    # main batch: H = 8, ten probes.  Second batch shape: H = 10, ONE probe (the hard key: no draw involved), where the bucket
    # histogram of the seeded data leaves 13 / 107 / 609 of the 4099 queries with fewer than 1 / 10 / 64 candidates (CPU oracle).
    for H, P, want_short in ((8, P_MAIN, None), (10, 1, True)):
        ix, q = _case(compat, H)
        ix.query_chunks = chunks
        try:
            want_rows, want_counts, n_short = _derived(ix, q, k, P, SEED)
            if want_short:
                assert 5 <= n_short <= Q // 4, n_short
            calls = _counting(monkeypatch)
            ix.query(q, k=k, hash_times=P, seed=SEED - 1)         # warm: task tables settled, one fill per range from here on
            calls.update(alloc=0, fill=0)
            rows, counts = _plain(ix.query(q, k=k, hash_times=P, seed=SEED))
            assert calls == {"alloc": 1, "fill": chunks}, calls
            assert counts == want_counts
            for qi, (got, want) in enumerate(zip(rows, want_rows)):
                assert got == want, (qi, got, want)
            old_rows, old_counts = _one_shot(monkeypatch, ix, q, k=k, hash_times=P, seed=SEED)
            assert calls == {"alloc": 1, "fill": chunks}
            assert old_counts == counts and old_rows == rows
        finally:
            ix.query_chunks = None
            monkeypatch.undo()


@pytest.mark.parametrize("chunks", [1, 2])
def test_first_call_with_a_task_table_retry_fills_once(monkeypatch, chunks):
    """A fresh indexer whose first task table is too small: every range overflows, its table is grown and the range repeated; the shells
    of the first attempt are kept and filled once, behind the settled launch.  Same seed, same lists on the second call."""
    from nlsh_amd.data import SIFT
    settled = _case(False, 8)[0]
    cg, q = _cases["data"]
    Ws, bs = synth.make_weights([D, 32, 8], seed=513)
    ix = ixmod.Indexer(make_hashing(D, [32], 8, Ws, bs, compat=False, seed=5), cg, SIFT.distance, compat=False)
    ix.query_chunks, ix._CHUNK_MIN_ROWS = chunks, 1024
    ix._estimate_tasks = lambda *a, **kw: 64
    calls = _counting(monkeypatch)
    first = _plain(ix.query(q, k=10, hash_times=P_MAIN, seed=SEED))
    assert min(ix._max_tasks.values()) > 64, "the case should overflow its first task table"
    assert calls == {"alloc": 1, "fill": chunks}, calls
    second = _plain(ix.query(q, k=10, hash_times=P_MAIN, seed=SEED))
    assert first == second
    assert first == _plain(settled.query(q, k=10, hash_times=P_MAIN, seed=SEED))


def test_opt_ins_give_equal_lists(monkeypatch):
    """`untracked_results` (rows off the collector, outer list on it) and `defer_result_release` (one range; the previous result is
    released in the window the shells would use, so that opt-in keeps the one-shot conversion) change no list."""
    ix, q = _case(True, 10)
    want = _plain(ix.query(q, k=10, hash_times=1, seed=SEED))
    calls = _counting(monkeypatch)
    monkeypatch.setattr(ixmod.Indexer, "untracked_results", True)
    rows, counts = ix.query(q, k=10, hash_times=1, seed=SEED)
    assert (rows, counts) == want and gc.is_tracked(rows)
    short = {qi for qi, n in enumerate(counts) if n < 10}          # rows replaced by the F7 rule are ordinary lists
    assert short and not any(gc.is_tracked(r) for qi, r in enumerate(rows) if qi not in short)
    monkeypatch.setattr(ixmod.Indexer, "untracked_results", False)
    monkeypatch.setattr(ixmod.Indexer, "defer_result_release", True)
    try:
        calls.update(alloc=0, fill=0)
        for _ in range(3):
            assert _plain(ix.query(q, k=10, hash_times=1, seed=SEED)) == want
        assert calls == {"alloc": 0, "fill": 0} and len(ix._held) <= 2
    finally:
        monkeypatch.setattr(ixmod.Indexer, "defer_result_release", False)
        ix._keep(([], []))
    monkeypatch.setattr(ixmod.Indexer, "promote_results", True)              # its one-shot bracket is kept: no shells
    calls.update(alloc=0, fill=0)
    assert ix.query(q, k=10, hash_times=1, seed=SEED) == want and calls == {"alloc": 0, "fill": 0}
