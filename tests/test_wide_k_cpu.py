"""k up to 256 in the tiled schedule and the top-k merges, the parts that need no device: the host-side validation of the C ABI,
the limits the facade and the header state, the oracle against the reference's recorded k = 100 / k = 200 lists, and the ISA lint of
the wide-k kernels (hipcc cross-compiles gfx950)."""
import ctypes
import json
import os
import re
import shutil
import sys

import numpy as np
import pytest

from helpers import G, cases
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402

needs_hipcc = pytest.mark.skipif(not (os.path.exists(isa_lint.HIPCC) or shutil.which("hipcc")), reason="hipcc not installed")


def _scan(L, algo, k, Q=0):
    """nlsh_scan_topk on an EMPTY batch (Q = 0): every argument check runs, nothing is launched and no pointer is read."""
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    return L.nlsh_scan_topk(a, 128, 128, a, a, a, None, 8, None, a, 128, Q, a, a, 10, k, 0, algo, 0, a, a, None, a, a, a, 4096, 16,
                            None, None, None)


def test_scan_topk_takes_wide_k_on_the_tiled_schedule_only():
    from nlsh_amd import _capi
    L = _capi.lib()
    for k in (1, 64, 65, 100, 256):
        assert _scan(L, 2, k) == _capi.OK, (k, L.nlsh_last_error())
    for algo in (0, 1):
        assert _scan(L, algo, 64) == _capi.OK
    for algo, k in ((2, 257), (2, 0), (0, 65), (1, 65), (0, 256), (1, 100)):
        assert _scan(L, algo, k) == _capi.E_UNSUPPORTED, (algo, k)
        msg = L.nlsh_last_error()
        # the refusal says which schedule takes which range, and names the remedy as the C ABI and as the facade spell it
        assert b"NLSH_SCAN_BUCKET_TILED" in msg and b'algo="tiled"' in msg and b"[1,64]" in msg and b"[1,256]" in msg, msg


def test_merge_topk_takes_k_up_to_256():
    from nlsh_amd import _capi
    L = _capi.lib()
    for k in (1, 64, 65, 100, 256):
        assert L.nlsh_merge_topk(None, k, 3, 0, k, None, None, None, None, None) == _capi.OK, (k, L.nlsh_last_error())
    assert L.nlsh_merge_topk(None, 300, 3, 0, 257, None, None, None, None, None) != _capi.OK
    assert b"256" in L.nlsh_last_error()
    assert L.nlsh_merge_topk(None, 99, 3, 0, 100, None, None, None, None, None) != _capi.OK      # row_stride < k


def test_step_descriptor_validates_k_through_the_same_rule():
    """nlsh_query_batch (and the step entry points, which share its scan call) refuse k = 65 on algo 1 and k = 257 on algo 2, and say why."""
    from nlsh_amd import _capi
    L = _capi.lib()
    dims = _capi.int_array([128, 64, 16])
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)

    def desc(**kw):
        base = dict(n_layers=2, act=0, key_mode=0, n_probes=10, dims=ctypes.cast(dims, ctypes.c_void_p), packed=a, n_multi_rows=0,
                    corpus_sorted=a, row_stride=128, gid=a, uniq_keys=a, offsets=a, bucket_order=a, cell_of=None, cell_offsets=None,
                    inv_norm=None, d=128, n_buckets=8, n_cells=0, k=10, metric=0, algo=2, seg_rows=0, hold_done=0, Q=64, qkeys=a, nkeys=a,
                    out_dist=a, out_idx=a, out_keys=None, out_ncand=a, status=a, workspace=a, workspace_bytes=4096, max_tasks=16,
                    front=None, plan=None, mid=None, tail=None)
        base.update(kw)
        return _capi.StepDesc(**base)
    # lookup_done = 1: the call goes straight to the scan's argument checks (no encoder launch in front of them)
    for kw in (dict(k=257), dict(k=65, algo=1)):
        d_ = desc(**kw)
        assert L.nlsh_query_batch(ctypes.byref(d_), ctypes.sizeof(d_), a, 128, 1, 0, 1, None, None, None) == _capi.E_UNSUPPORTED, kw
        assert b"NLSH_SCAN_BUCKET_TILED" in L.nlsh_last_error()


def test_limits_in_the_facade_and_the_header():
    from nlsh_amd import _capi
    assert _capi.MAX_K == 64 and _capi.MAX_K_TILED == 256
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    assert re.search(r"#define NLSH_MAX_K 64\b", header) and re.search(r"#define NLSH_MAX_K_TILED 256\b", header)
    assert re.search(r"#define NLSH_ABI_VERSION 4\b", header) and _capi.lib().nlsh_abi_version() == 4   # a relaxed limit: no new ABI


@pytest.mark.parametrize("name", ["l2_k100", "cos_k200"])
def test_g9_query_widek_oracle(name):
    """The oracle against the reference's Indexer.query at k = 100 / 200 (the assertions of test_g5_query_injected_keys)."""
    meta = json.load(open(os.path.join(G, "g9_query_widek.json")))[name]
    g = np.load(os.path.join(G, "g9_query_widek.npz"))
    corpus, queries, Ws, bs = cases.g5_inputs(meta)
    ox = oracle.OracleIndexer(Ws, bs, corpus, metric=meta["metric"], act="tanh" if meta["metric"] == "cosine" else "sigmoid")
    assert (ox.corpus_keys == g[name + "/corpus_keys"]).mean() > 0.999
    ox.corpus_keys = g[name + "/corpus_keys"].astype(np.int64)
    ox.perm, ox.uniq_keys, ox.offsets = oracle.build_csr(ox.corpus_keys)
    res, nc, od, oi = ox.query_with_keys(queries, meta["injected_iter"], k=meta["k"])
    assert nc == g[name + "/ncand"].tolist()
    assert sum(c >= meta["k"] for c in nc) >= 9 and 0 in nc and any(0 < c < meta["k"] for c in nc)   # full lists, empty ones and F7
    off = g[name + "/cand_off"]
    tol = 1e-4
    for q in range(meta["Q"]):
        rows = g[name + "/cand_rows"][off[q]:off[q + 1]]
        dref = g[name + "/cand_dist"][off[q]:off[q + 1]]
        d32, d64 = oracle.distances(queries[q], corpus, rows, meta["metric"], f64=True)
        assert np.all(np.abs(d32 - dref) <= tol * np.maximum(1.0, np.abs(dref)))
        assert np.all(np.abs(d64 - dref) <= tol * np.maximum(1.0, np.abs(dref)))
        ref_ids = meta["result_ids"][q]
        if nc[q] < meta["k"]:
            assert res[q] == ref_ids                                    # F7 fallback: exact list
            continue
        cases.assert_topk_equivalent(res[q], ref_ids, rows, dref, meta["k"], tol)
    rec = oracle.calculate_recall(list(g[name + "/ground_truth"]), res)
    assert np.allclose(rec, g[name + "/recalls"], atol=1.0 / meta["k"] + 1e-9)
    assert abs(np.mean(rec) - meta["mean_recall"]) < 0.02


@needs_hipcc
def test_wide_tiled_scan_kernels_are_clean():
    """bscanw_kernel = the tiled task body with the wide epilogue: the same hand-placed scalar loads, so the same lint; and the budget
    of its first clean compile (70 VGPRs, 7 waves per SIMD, the 20 KB tile: what the k <= 64 kernels have) as bounds."""
    rep = isa_lint.lint("scan_bucket.hip", "bscanw_kernel")
    assert len(rep) == 3, sorted(rep)                      # L2 (exact), L2 (folded eps) and cosine
    for name, r in rep.items():
        assert r["scalar_loads"] > 100, name
        assert r["violations"] == [], (name, r["violations"][:5])
        res = r["resources"]
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (name, res)
        assert not [x for x in r["hot_loop_spills"] if x.startswith("v_writelane")], (name, r["hot_loop_spills"][:5])
        assert len(r["hot_loop_spills"]) <= 4, (name, r["hot_loop_spills"][:8])
        assert res["SGPRs Spill"] <= 32, (name, res)
        assert res["Occupancy"] >= 7 and res["VGPRs"] <= 72, (name, res)
        assert res["LDS Size"] <= 20480, (name, res)


@needs_hipcc
def test_wide_merge_kernels_are_clean():
    """The wide merges (2, 3, 4 keys per lane): no scratch, no spills, 8 waves per SIMD; LDS = 4 waves x 256 keys of scratch (8 KB),
    plus the 4 KB list table in the scan's merge."""
    for src, sym, lds in (("scan_bucket.hip", "bmergew_kernel", 12288), ("scan_topk.hip", "merge_shards_wide_kernel", 8192)):
        rep = isa_lint.lint(src, sym)
        assert len(rep) == 3, sorted(rep)
        for name, r in rep.items():
            res = r["resources"]
            assert r["violations"] == [], (name, r["violations"][:5])
            assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, (name, res)
            assert res["Occupancy"] >= 8 and res["VGPRs"] <= 64, (name, res)
            assert res["LDS Size"] <= lds, (name, res)

