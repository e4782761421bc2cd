"""Radius queries, the part that needs no device: the new C-ABI symbols, the workspace-size functions, every host-side refusal of
`nlsh_range_count` / `nlsh_range_fill` (code + the argument's name in the message, before anything is launched) and of the facade, the
lint of the new kernels, and the numpy statement of the definition the GPU tests use as their reference (a cut on the distance, a sort
by the 64-bit key) against a brute-force float64 ordering.  No call here reaches a device: the pointers are made-up addresses that a
refused call never reads."""
import os
import re

import numpy as np
import pytest
import torch

from nlsh_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nlsh_range_workspace", "nlsh_range_sort_workspace", "nlsh_range_count", "nlsh_range_fill")
FAKE = 0x10000          # a 16-byte aligned non-null address: refused calls never dereference it


def _lib():
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build_library()
    return _capi.lib()


def _err():
    return _lib().nlsh_last_error().decode()


def test_new_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    declared = set(re.findall(r"\b(nlsh_[a-z0-9_]+)\s*\(", header))
    L = _lib()
    for sym in NEW:
        assert sym in declared and sym in _capi.SYMBOLS and hasattr(L, sym), sym
    assert L.nlsh_abi_version() == 4            # the change only adds entry points


def test_workspace_sizes_are_monotone():
    L = _lib()
    base = dict(Q=100, P=4, max_tasks=1000, n_buckets=50, d=100)
    size = lambda **kw: L.nlsh_range_workspace(*[{**base, **kw}[n] for n in ("Q", "P", "max_tasks", "n_buckets", "d")])      # noqa: E731
    assert size() > 0
    for name, values in (("Q", (0, 1, 100, 1000, 10 ** 5)), ("P", (1, 2, 8, 64)), ("max_tasks", (0, 1, 10 ** 3, 10 ** 6)),
                         ("n_buckets", (0, 1, 50, 10 ** 5)), ("d", (1, 3, 4, 100, 1024))):
        got = [size(**{name: v}) for v in values]
        assert all(a <= b for a, b in zip(got, got[1:])) and got[0] > 0, (name, got)
    # the plan of a k = 1 call: what the top-k call takes at k = 1, and never more than at k = 10
    assert size() <= L.nlsh_scan_workspace(100, 4, 1, 1000, 50, 100) < L.nlsh_scan_workspace(100, 4, 10, 1000, 50, 100)
    for bad in (dict(Q=-1), dict(P=0), dict(max_tasks=-1), dict(n_buckets=-1), dict(d=0)):
        assert size(**bad) == 0 and "range_workspace" in _err(), bad
    totals = (0, 1, 255, 256, 257, 10 ** 4, 10 ** 6)
    got = [L.nlsh_range_sort_workspace(64, t) for t in totals]
    assert all(a <= b for a, b in zip(got, got[1:])) and got[0] > 0, got
    assert all(g >= 2 * 8 * t for g, t in zip(got, totals))       # the unsorted and the sorted keys
    assert L.nlsh_range_sort_workspace(0, 0) > 0
    for bad in ((-1, 0), (1, -1), (1, 2 ** 31)):
        assert L.nlsh_range_sort_workspace(*bad) == 0 and "total" in _err(), bad


def _count(algo=_capi.SCAN_BUCKET_TILED, storage=_capi.STORE_F32, row_stride=8, d=8, Q=4, P=2, n_buckets=3, max_tasks=16, row_filter=None,
           radius=FAKE, out_count=FAKE, out_ncand=FAKE, workspace_bytes=0, metric=_capi.METRIC_L2_EPS):
    return _lib().nlsh_range_count(FAKE, storage, row_stride, d, FAKE, FAKE, FAKE, None, n_buckets, None, None, 0, None, FAKE, d, Q, FAKE, FAKE, P,
                                   metric, algo, row_filter, radius, out_count, out_ncand, FAKE, FAKE, workspace_bytes, max_tasks, None, None, None)


def _fill(algo=_capi.SCAN_BUCKET_TILED, storage=_capi.STORE_F32, row_stride=8, d=8, Q=4, P=2, n_buckets=3, max_tasks=16, row_filter=None,
          radius=FAKE, row_offsets=FAKE, total=5, cursor=FAKE, out_keys=None, out_dist=None, out_idx=FAKE, workspace_bytes=0,
          sort_workspace=FAKE, sort_bytes=0):
    return _lib().nlsh_range_fill(FAKE, storage, row_stride, d, FAKE, FAKE, FAKE, None, n_buckets, None, None, 0, None, FAKE, d, Q, FAKE, FAKE, P,
                                  _capi.METRIC_L2_EPS, algo, row_filter, radius, row_offsets, total, cursor, out_keys, out_dist, out_idx,
                                  FAKE, FAKE, workspace_bytes, max_tasks, sort_workspace, sort_bytes, None, None, None)


@pytest.mark.parametrize("call", [_count, _fill])
def test_refusals_common_to_both_calls(call):
    for algo in (_capi.SCAN_QUERY_MAJOR, _capi.SCAN_BUCKET_MAJOR):          # the range epilogue is the tiled schedule's alone
        assert call(algo=algo) == _capi.E_UNSUPPORTED and "algo" in _err() and "tiled" in _err()
    assert call(algo=9) == _capi.E_INVALID and "algo" in _err()
    assert call(radius=None) == _capi.E_INVALID and "radius" in _err()
    assert call(row_filter=FAKE + 2) == _capi.E_INVALID and "row_filter" in _err()
    assert call(P=_capi.MAX_PROBES + 1) == _capi.E_UNSUPPORTED and "P=" in _err()
    assert call(P=0) == _capi.E_UNSUPPORTED and "P=" in _err()
    assert call(d=_capi.MAX_DIM + 1, row_stride=_capi.MAX_DIM + 4) == _capi.E_UNSUPPORTED and "d=" in _err()
    assert call(Q=-1) == _capi.E_INVALID and "Q=" in _err()
    assert call(n_buckets=-1) == _capi.E_INVALID and "n_buckets" in _err()
    assert call(max_tasks=-1) == _capi.E_INVALID and "max_tasks" in _err()
    assert call(storage=7) == _capi.E_INVALID and "storage" in _err()
    assert call(storage=_capi.STORE_F16, row_stride=12) == _capi.E_INVALID and "row_stride" in _err()
    # the workspace (0 bytes) is too small: every check of the arguments passed, and still nothing was launched
    assert call() == _capi.E_WORKSPACE


def test_refusals_of_each_call():
    assert _count(out_count=None) == _capi.E_INVALID and "out_count" in _err()
    assert _count(out_ncand=None) == _capi.E_INVALID and "out_ncand" in _err()
    assert _count(Q=0, out_count=None) == _capi.E_INVALID and "out_count" in _err()
    assert _count(Q=0) == _capi.OK                                           # an empty batch: valid, nothing launched
    assert _fill(row_offsets=None) == _capi.E_INVALID and "row_offsets" in _err()
    assert _fill(row_offsets=FAKE + 4) == _capi.E_INVALID and "row_offsets" in _err()
    assert _fill(total=-1) == _capi.E_INVALID and "total" in _err()
    assert _fill(total=2 ** 31) == _capi.E_INVALID and "total" in _err()
    assert _fill(cursor=None) == _capi.E_INVALID and "cursor" in _err()
    assert _fill(out_idx=None) == _capi.E_INVALID and "out_idx" in _err()
    assert _fill(sort_workspace=None) == _capi.E_WORKSPACE and "sort_workspace" in _err()
    assert _fill(Q=0, total=0) == _capi.OK


def test_range_kernels_are_clean():
    """bscanr_kernel = the tiled task body with the range epilogue: the same hand-placed scalar loads, so the same lint (no instruction
    may name an SGPR a scalar load in flight still owns); 9 instantiations (3 storages x 3 metrics: mode and filter are run-time
    operands), no scratch, no VGPR spill, the 20 KB tile and no LDS beyond it."""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    if not (os.path.exists(isa_lint.HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not installed")
    rep = isa_lint.lint("scan_bucket_range.hip", "bscanr_kernel")
    assert len(rep) == 9, sorted(rep)
    for name, r in rep.items():
        res = r["resources"]
        assert r["scalar_loads"] > 100, name
        assert r["violations"] == [], (name, r["violations"][:5])
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (name, res)
        assert not [x for x in r["hot_loop_spills"] if x.startswith("v_writelane")], (name, r["hot_loop_spills"][:5])
        assert res["Occupancy"] >= 6 and res["VGPRs"] <= 80 and res["LDS Size"] == 20480, (name, res)


def _bare_indexer(metric="l2"):
    from nlsh_amd.indexer import Indexer
    ix = Indexer.__new__(Indexer)           # the validation below runs before the index's arrays are touched
    ix.metric, ix.algo, ix.generation = metric, None, 0
    return ix


def test_radius_validation():
    from nlsh_amd.indexer import Indexer
    cpu = torch.device("cpu")
    r = Indexer._checked_radius(1.5, 3, cpu)
    assert r.dtype == torch.float32 and r.tolist() == [1.5] * 3
    assert Indexer._checked_radius(0.1, 1, cpu).item() == float(np.float32(0.1))
    assert Indexer._checked_radius(float("inf"), 2, cpu).tolist() == [float("inf")] * 2
    assert Indexer._checked_radius(1e300, 1, cpu).item() == float("inf")         # beyond float32: the float32 it rounds to
    assert Indexer._checked_radius(-1, 2, cpu).tolist() == [-1.0, -1.0]
    t = torch.tensor([0.0, -1.0, float("inf")])
    assert Indexer._checked_radius(t, 3, cpu) is t
    for bad in (float("nan"), torch.tensor([1.0, float("nan"), 2.0])):
        with pytest.raises(ValueError, match="NaN"):
            Indexer._checked_radius(bad, 3, cpu)
    for bad in (torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float16), torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="float32"):
            Indexer._checked_radius(bad, 3, cpu)
    for bad in (torch.zeros(2), torch.zeros(4), torch.zeros((3, 1)), torch.zeros(())):
        with pytest.raises(ValueError, match="one value per query"):
            Indexer._checked_radius(bad, 3, cpu)
    with pytest.raises(ValueError, match="is on"):
        Indexer._checked_radius(torch.zeros(3), 3, torch.device("meta"))
    for bad in (None, "1.0", True, [1.0], 1j):
        with pytest.raises(ValueError, match="Python float"):
            Indexer._checked_radius(bad, 3, cpu)


def test_facade_refusals_before_any_launch():
    from nlsh_amd.indexer import RowFilter
    ix, other = _bare_indexer(), _bare_indexer()
    theirs = RowFilter(other, None, 0, 0)
    stale = RowFilter(ix, None, 0, -1)
    calls = {
        "range_scan_tensors": lambda **kw: ix.range_scan_tensors(None, None, None, 1.0, **kw),
        "range_tensors": lambda **kw: ix.range_tensors(None, 1.0, **kw),
        "range_query": lambda **kw: ix.range_query(None, 1.0, **kw),
        "range_query_with_keys": lambda **kw: ix.range_query_with_keys(None, [], 1.0, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="another index"):
            call(filter=theirs)
        with pytest.raises(ValueError, match="stale"):
            call(filter=stale)
    for name in ("range_tensors", "range_query"):
        with pytest.raises(ValueError, match="hash_times"):
            calls[name](hash_times=65)
    generic = _bare_indexer("generic")
    for call in (lambda: generic.range_scan_tensors(None, None, None, 1.0), lambda: generic.range_tensors(None, 1.0),
                 lambda: generic.range_query(None, 1.0)):
        with pytest.raises(NotImplementedError):
            call()
    # host queries: there is no CPU path
    with pytest.raises(_capi.NlshHipError, match="device-resident"):
        ix.range_scan_tensors(torch.zeros((2, 4)), torch.zeros((2, 1), dtype=torch.int32), torch.ones(2, dtype=torch.int32), 1.0)


# ---------------------------------------------------------------------------------------------- the definition, in numpy
def mono(dist):
    """float32 [n] -> uint32 [n]: the order-preserving word of the sort key (csrc/common.h mono_from_float)."""
    bits = np.asarray(dist, np.float32).view(np.uint32)
    return np.where(bits & 0x80000000, ~bits, bits | 0x80000000).astype(np.uint32)


def range_reference(dist, ids, radius):
    """The definition on one query's candidates: the cut `dist <= radius` in float32 (a NaN never passes) and the sort by
    mono(dist) << 32 | id -> (ids, dist, keys64), what the GPU tests hold the range result against."""
    dist, ids = np.asarray(dist, np.float32), np.asarray(ids, np.int32)
    with np.errstate(invalid="ignore"):
        keep = dist <= np.float32(radius)
    key = (mono(dist[keep]).astype(np.uint64) << np.uint64(32)) | ids[keep].view(np.uint32).astype(np.uint64)
    order = np.argsort(key, kind="stable")
    return ids[keep][order], dist[keep][order], key[order]


def test_numpy_definition_against_a_brute_force_ordering():
    rng = np.random.default_rng(11)
    for n in (0, 1, 7, 200):
        for _ in range(4):
            q = rng.integers(-3, 4, size=6).astype(np.float64)
            rows = rng.integers(-3, 4, size=(n, 6)).astype(np.float64)          # small integers: mass ties, float32 sums exact
            d64 = np.sqrt(((q - rows) ** 2).sum(1))
            d32 = d64.astype(np.float32)
            ids = rng.permutation(np.arange(-n, n))[:n].astype(np.int32)          # negative ids: ties come out in unsigned id order
            for radius in ([0.0, -1.0, np.inf] + ([float(d32[n // 2]), float(np.nextafter(d32[n // 2], np.float32(-np.inf)))] if n else [])):
                got_ids, got_d, got_k = range_reference(d32, ids, radius)
                want = sorted((float(d32[i]), int(np.uint32(ids[i])), int(ids[i])) for i in range(n) if float(d32[i]) <= float(np.float32(radius)))
                assert got_ids.tolist() == [w[2] for w in want], (n, radius)
                assert got_d.tolist() == [w[0] for w in want]
                assert np.all(got_k[1:] > got_k[:-1])                           # distinct keys, ascending
                # float64 agrees on which rows are in range: the distances of integer data are exact or correctly rounded
                assert len(want) == int((d64.astype(np.float32) <= np.float32(radius)).sum())
    # non-finite distances: a NaN is never in range, +inf only at +inf, -0.0 sorts with +0.0's neighbours by its own word
    d = np.asarray([np.nan, np.inf, 1.0, -0.0, 0.0], np.float32)
    ids = np.arange(5, dtype=np.int32)
    assert range_reference(d, ids, np.inf)[0].tolist() == [3, 4, 2, 1]
    assert range_reference(d, ids, 3e38)[0].tolist() == [3, 4, 2]
    assert range_reference(d, ids, -1.0)[0].tolist() == []
