"""Row filters, the part that needs no device: the new C-ABI symbols, `nlsh_row_filter_words`, every host-side refusal of
`nlsh_row_filter_build` and `nlsh_scan_topk_cells_phase_filtered` (code + the argument's name in the message, before anything is
launched), `Indexer.row_filter`'s argument validation, and the packing rule the GPU tests use as their reference
(`nlsh_amd.indexer.pack_row_filter`) against a bit-by-bit loop.  No call here reaches a device: the pointers are made-up addresses
that a refused call never reads."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from nlsh_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nlsh_row_filter_words", "nlsh_row_filter_build", "nlsh_scan_topk_cells_phase_filtered")
SIZES = (0, 1, 31, 32, 33, 63, 64, 65, 20000)
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


def test_row_filter_words():
    L = _lib()
    for n in SIZES + (2 ** 31 - 1,):
        assert L.nlsh_row_filter_words(n) == 2 * ((n + 63) // 64), n
    assert L.nlsh_row_filter_words(-1) == 0 and "n_rows" in _err()


def pack_loop(allowed):
    """The layout, one bit at a time: bit p & 31 of word p >> 5 is sorted row p; 2 * ceil(N / 64) words; the tail is zero."""
    n = len(allowed)
    words = [0] * (2 * ((n + 63) // 64))
    for p, a in enumerate(allowed):
        if a:
            words[p >> 5] |= 1 << (p & 31)
    return np.asarray(words, dtype=np.uint32)


def test_packing_rule_against_a_bit_loop():
    from nlsh_amd.indexer import pack_row_filter
    rng = np.random.default_rng(5)
    for n in SIZES[:-1] + (127, 128, 129, 1000):
        for allowed in (rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool), np.arange(n) % 2 == 0, np.arange(n) == n - 1):
            got = pack_row_filter(allowed)
            assert got.dtype == np.uint32 and np.array_equal(got, pack_loop(allowed)), n
            assert int(sum(bin(int(w)).count("1") for w in got)) == int(np.sum(allowed))


def _build(gid=FAKE, n_rows=64, ids=None, n_ids=0, dense=None, n_dense=0, id_base=0, invert=0, row_filter=FAKE, n_allowed=FAKE):
    return _lib().nlsh_row_filter_build(gid, n_rows, ids, n_ids, dense, n_dense, id_base, invert, row_filter, n_allowed, None)


@pytest.mark.parametrize("kwargs, name", [
    (dict(ids=FAKE, n_rows=-1), "n_rows"),
    (dict(ids=FAKE, n_rows=2 ** 31), "n_rows"),
    (dict(ids=FAKE, dense=FAKE), "both ids and dense"),
    (dict(), "neither ids nor dense"),
    (dict(ids=FAKE, n_ids=-1), "n_ids"),
    (dict(dense=FAKE, n_dense=-1), "n_dense"),
    (dict(ids=FAKE, invert=2), "invert"),
    (dict(ids=FAKE, n_allowed=None), "n_allowed"),
    (dict(ids=FAKE, gid=None), "gid"),
    (dict(ids=FAKE, row_filter=None), "row_filter"),
    (dict(ids=FAKE, row_filter=FAKE + 2), "row_filter"),
    (dict(ids=FAKE, n_allowed=FAKE + 1), "n_allowed"),
])
def test_row_filter_build_refusals(kwargs, name):
    assert _build(**kwargs) == _capi.E_INVALID
    assert name in _err(), _err()


def _filtered(algo=_capi.SCAN_BUCKET_TILED, storage=_capi.STORE_F32, row_stride=8, row_filter=FAKE, phases=_capi.PHASE_ALL, corpus=FAKE):
    d, Q, P, k = 8, 4, 2, 10
    return _lib().nlsh_scan_topk_cells_phase_filtered(
        corpus, storage, row_stride, d, FAKE, FAKE, FAKE, None, 3, None, None, 0, None, FAKE, d, Q, FAKE, FAKE, P, k,
        _capi.METRIC_L2_EPS, algo, 0, FAKE, FAKE, None, FAKE, FAKE, FAKE, 0, 16, None, None, None, phases, row_filter)


def test_filtered_scan_refusals():
    for algo in (_capi.SCAN_QUERY_MAJOR, _capi.SCAN_BUCKET_MAJOR):          # a filter is the tiled schedule's alone
        assert _filtered(algo=algo) == _capi.E_UNSUPPORTED
        assert "row_filter" in _err() and "tiled" in _err()
    assert _filtered(row_filter=FAKE + 2) == _capi.E_INVALID and "row_filter" in _err()
    assert _filtered(storage=7) == _capi.E_INVALID and "storage" in _err()
    assert _filtered(algo=9) == _capi.E_INVALID and "algo" in _err()
    assert _filtered(phases=0) == _capi.E_INVALID and "phases" in _err()
    assert _filtered(storage=_capi.STORE_F16, row_stride=12) == _capi.E_INVALID and "row_stride" in _err()
    # the workspace (0 bytes) is too small: every check of the arguments passed, and still nothing was launched
    assert _filtered() == _capi.E_WORKSPACE
    # a null filter is the typed call: its refusal of a compressed corpus outside the tiled schedule, in its words
    assert _filtered(algo=_capi.SCAN_QUERY_MAJOR, storage=_capi.STORE_U8, row_stride=16, row_filter=None) == _capi.E_UNSUPPORTED
    assert "scan_topk_typed" in _err()


def test_filtered_scan_kernels_are_clean():
    """bscanf_kernel = the tiled task body with the filter's bit in its epilogue: the same hand-placed scalar loads, so the same lint (no
    instruction may name an SGPR a scalar load in flight still owns); 18 instantiations (3 storages x 3 metrics x narrow / wide k), no
    scratch, no VGPR spill, the 20 KB tile.  The four filter words are four VGPRs: the float32 kernels may drop one wave per SIMD."""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    if not (os.path.exists(isa_lint.HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not installed")
    rep = isa_lint.lint("scan_bucket_filtered.hip", "bscanf_kernel")
    assert len(rep) == 18, sorted(rep)
    for name, r in rep.items():
        res = r["resources"]
        assert r["scalar_loads"] > 100, name
        assert r["violations"] == [], (name, r["violations"][:5])
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (name, res)
        assert not [x for x in r["hot_loop_spills"] if x.startswith("v_writelane")], (name, r["hot_loop_spills"][:5])
        assert res["Occupancy"] >= 6 and res["VGPRs"] <= 80 and res["LDS Size"] <= 20480, (name, res)


def _bare_indexer(metric="l2"):
    from nlsh_amd.indexer import Indexer
    ix = Indexer.__new__(Indexer)           # the validation below runs before the index's arrays are touched
    ix.metric, ix.algo, ix.generation = metric, None, 0
    return ix


def test_row_filter_argument_validation():
    ix = _bare_indexer()
    for kwargs in ({}, dict(allow=[1], deny=[2]), dict(allow=[1], mask=torch.zeros(4, dtype=torch.bool)),
                   dict(allow=[1], deny=[2], mask=torch.zeros(4, dtype=torch.bool))):
        with pytest.raises(ValueError, match="exactly one"):
            ix.row_filter(**kwargs)
    for bad in ([1.5], [True], torch.tensor([1.0]), torch.tensor([True]), ["a"]):
        with pytest.raises(ValueError, match="integer ids"):
            ix.row_filter(allow=bad)
        with pytest.raises(ValueError, match="integer ids"):
            ix.row_filter(deny=bad)
    for bad in ([1, 0, 1], torch.zeros(4, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.bool)):
        with pytest.raises(ValueError, match="mask"):
            ix.row_filter(mask=bad)
    with pytest.raises(_capi.NlshHipError, match="device-resident"):
        ix.row_filter(mask=torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        _bare_indexer("generic").row_filter(allow=[1])


def test_filter_argument_refusals_before_any_launch():
    from nlsh_amd.indexer import RowFilter
    ix, other = _bare_indexer(), _bare_indexer()
    mine, theirs = RowFilter(ix, None, 0, 0), RowFilter(other, None, 0, 0)
    assert ix._checked_filter(None) is None and ix._checked_filter(mine) is mine
    with pytest.raises(ValueError, match="RowFilter"):
        ix._checked_filter(torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="another index"):
        ix._checked_filter(theirs)
    ix.generation = 1
    with pytest.raises(ValueError, match="stale"):
        ix._checked_filter(mine)
    ix.generation = 0
    for forced in ("query", "bucket"):
        ix.algo = forced
        with pytest.raises(ValueError, match="tiled"):
            ix._checked_filter(mine)
    ix.algo = "tiled"
    assert ix._checked_filter(mine) is mine
    with pytest.raises(ValueError, match="tiled"):
        ix._checked_filter(mine, algo=_capi.SCAN_QUERY_MAJOR)
    ix.metric = "generic"
    with pytest.raises(NotImplementedError):
        ix._checked_filter(mine)
    # the public calls check the filter first: nothing of the (absent) index arrays is touched before the refusal
    for call in (lambda: ix.query(None, filter=theirs), lambda: ix.query_tensors(None, filter=theirs),
                 lambda: ix.scan_tensors(None, None, None, filter=theirs), lambda: ix.query_with_keys(None, [], filter=theirs)):
        with pytest.raises(ValueError, match="another index"):
            call()
