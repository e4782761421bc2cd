"""sq8 corpus storage (per-dimension affine uint8), the parts that need no device: the rule restated in numpy -- `sq8_train`,
`sq8_encode`, `sq8_decode` below are the reference of the GPU tests (tests/test_gpu_sq8_storage.py imports them) --, the five exports
against the header and the binding, every host-side refusal of the new calls (nothing is launched and no pointer is read before the
checks pass), the facade's refusals, and the resource figures of the affine scan kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, U8 = 0, 1, 2


# ---------------------------------------------------------------------------------------------- the rule
def sq8_train(x):
    """(lo, step) float32 [d] of rows [N, d]: lo = min + 0.0f, hi = max + 0.0f (a zero of either sign becomes +0),
    step = (hi - lo) / 255.0f, or 1.0f where hi == lo.  Finite rows only."""
    x = np.asarray(x).astype(np.float32)
    assert np.isfinite(x).all()
    zero = np.float32(0.0)
    lo = (x.min(axis=0) + zero).astype(np.float32)
    hi = (x.max(axis=0) + zero).astype(np.float32)
    with np.errstate(over="ignore"):
        step = ((hi - lo).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    return lo, np.where(hi == lo, np.float32(1.0), step).astype(np.float32)


def sq8_encode(x, lo, step):
    """codes uint8 of finite float32 x: t = (x - lo) / step as an IEEE subtract and a correctly rounded divide, rint (half to even),
    clamped to [0, 255] -> (codes, per-row flag "at least one element saturated")."""
    x = np.asarray(x).astype(np.float32)
    assert np.isfinite(x).all()
    with np.errstate(over="ignore"):
        t = ((x - lo).astype(np.float32) / step).astype(np.float32)
    r = np.rint(t)
    clamped = ((r < 0) | (r > 255)).reshape(x.shape[0], -1).any(axis=1) if x.ndim == 2 else ((r < 0) | (r > 255))
    return np.clip(r, 0, 255).astype(np.uint8), clamped


def sq8_decode(codes, lo, step):
    """deq(c, j) = float(c) * step[j] + lo[j]: two roundings, no fused multiply-add."""
    prod = (np.asarray(codes).astype(np.float32) * step).astype(np.float32)
    return (prod + lo).astype(np.float32)


def test_the_rule_is_the_torch_expression_in_every_bit():
    import torch
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((500, 37)) * rng.uniform(0.01, 30, size=37) + rng.uniform(-5, 5, size=37)).astype(np.float32)
    lo, step = sq8_train(x)
    codes, _ = sq8_encode(x, lo, step)
    tx, tlo, tstep = torch.from_numpy(x), torch.from_numpy(lo), torch.from_numpy(step)
    tcodes = ((tx - tlo) / tstep).round().clamp(0, 255).to(torch.uint8)
    assert np.array_equal(tcodes.numpy(), codes)
    assert np.array_equal((tcodes.float() * tstep + tlo).numpy().view(np.int32), sq8_decode(codes, lo, step).view(np.int32))
    assert codes.min() == 0 and codes.max() == 255
    # the round trip stays within half a step per dimension (and a float32 rounding of the rule's own operations)
    err = np.linalg.norm(x.astype(np.float64) - sq8_decode(codes, lo, step), axis=1)
    assert (err <= 0.5 * np.linalg.norm(step.astype(np.float64)) * (1 + 1e-4)).all()


def test_identity_quantiser_is_uint8_storage():
    v = np.arange(256, dtype=np.float32).reshape(16, 16)
    lo, step = np.zeros(16, np.float32), np.ones(16, np.float32)
    codes, clamped = sq8_encode(v, lo, step)
    assert np.array_equal(codes, v.astype(np.uint8)) and not clamped.any()
    assert np.array_equal(sq8_decode(codes, lo, step).view(np.int32), v.view(np.int32))


def test_saturation_at_both_ends_is_counted_not_refused():
    lo, step = np.array([-1.0, 10.0], np.float32), np.array([0.5, 2.0], np.float32)
    x = np.array([[-1.0, 10.0], [126.5, 520.0], [-1.26, 9.0], [126.76, 521.1], [-1e30, 1e30], [3.4e38, -3.4e38]], np.float32)
    codes, clamped = sq8_encode(x, lo, step)
    assert codes.tolist() == [[0, 0], [255, 255], [0, 0], [255, 255], [0, 255], [255, 0]]
    assert clamped.tolist() == [False, False, True, True, True, True]       # -1.26 -> rint(-0.52) = -1: below; 9.0 -> -0.5 -> -0: inside


def test_ties_round_to_even():
    lo, step = np.zeros(1, np.float32), np.full(1, 2.0, np.float32)
    x = np.array([[1.0], [3.0], [5.0], [7.0], [509.0], [0.999999], [1.000001]], np.float32)      # t = 0.5, 1.5, 2.5, 3.5, 254.5, ...
    assert sq8_encode(x, lo, step)[0].reshape(-1).tolist() == [0, 2, 2, 4, 254, 0, 1]


def test_a_constant_column_trains_step_one():
    x = np.stack([np.full(9, 3.25, np.float32), np.arange(9, dtype=np.float32)], axis=1)
    lo, step = sq8_train(x)
    assert lo.tolist() == [3.25, 0.0] and step.tolist() == [1.0, np.float32(8.0) / np.float32(255.0)]
    codes, clamped = sq8_encode(x, lo, step)
    assert codes[:, 0].tolist() == [0] * 9 and codes[[0, -1], 1].tolist() == [0, 255] and not clamped.any()
    assert np.array_equal(sq8_decode(codes, lo, step)[:, 0], x[:, 0])


def test_signed_zeros_train_to_plus_zero():
    for col in ([-0.0, -0.0, -0.0], [-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, -2.0, -1.0], [-0.0, 2.0, 1.0]):
        x = np.array(col, np.float32).reshape(-1, 1)
        lo, step = sq8_train(x)
        lo_bits, hi = lo.view(np.int32)[0], np.float32(max(col)) + np.float32(0.0)
        if min(col) == 0:
            assert lo_bits == 0, col                                      # +0, never the bits of -0
        assert not np.signbit(hi)
        assert step[0] == (1.0 if max(col) == min(col) else np.float32(2.0) / np.float32(255.0))
        assert sq8_encode(x, lo, step)[0][0, 0] == (0 if min(col) == 0 else 255)      # either zero is the same code


# ---------------------------------------------------------------------------------------------- the C ABI, host side
@pytest.fixture(scope="module")
def L():
    from nlsh_amd import _capi
    return _capi.lib()


SQ8 = ("nlsh_sq8_train_workspace", "nlsh_sq8_train", "nlsh_gather_rows_sq8", "nlsh_csr_update_sq8", "nlsh_scan_topk_cells_phase_sq8")


def test_sq8_exports_exist_and_header_binding_and_library_agree(L):
    from nlsh_amd import _capi
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    for sym in SQ8:
        assert sym in _capi.SYMBOLS and hasattr(L, sym)
        decl = re.search(r"(?:int|size_t) %s\((.*?)\);" % sym, header, re.S)
        assert decl, sym
        assert len(getattr(L, sym).argtypes) == len(decl.group(1).split(",")), sym
    # an sq8 call is its typed twin with (lo, step) where the storage code stood (and clamped_rows behind first_bad)
    assert len(L.nlsh_scan_topk_cells_phase_sq8.argtypes) == len(L.nlsh_scan_topk_cells_phase_filtered.argtypes) + 1
    assert len(L.nlsh_gather_rows_sq8.argtypes) == len(L.nlsh_gather_rows_typed.argtypes) + 2
    assert len(L.nlsh_csr_update_sq8.argtypes) == len(L.nlsh_csr_update_typed.argtypes) + 2
    # the ABI did not move, and sq8 is no fourth storage code
    assert int(re.search(r"#define NLSH_ABI_VERSION (\d+)", header).group(1)) == 4 and L.nlsh_abi_version() == 4
    assert not re.search(r"#define NLSH_STORE_\w+ 3", header)
    assert "storage" not in [f[0] for f in _capi.StepDesc._fields_]


def _buf():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 255) & ~255


def _scan(L, algo=2, row_stride=128, d=128, k=10, null=(), misalign=(), ws_bytes=None, Q=4, P=2, max_tasks=64, nb=3, phases=7):
    """nlsh_scan_topk_cells_phase_sq8 with pointers into a small host buffer: every call here must be refused before any is used."""
    keep, a = _buf()
    need = L.nlsh_scan_workspace(Q, P, k, max_tasks, nb, d)
    p = lambda name: None if name in null else a + 4 if name in misalign else a   # noqa: E731
    return L.nlsh_scan_topk_cells_phase_sq8(
        p("corpus_sorted"), p("lo"), p("step"), row_stride, d, p("gid"), p("uniq_keys"), p("offsets"), None, nb, None, None, 0, p("inv_norm"),
        p("queries"), d, Q, p("qkeys"), p("nkeys"), P, k, 0, algo, 0, p("out_dist"), p("out_idx"), None, p("out_ncand"), p("status"),
        p("workspace"), need if ws_bytes is None else ws_bytes, max_tasks, None, None, None, phases, None)


def test_sq8_scan_refuses_on_the_host(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731
    for algo in (0, 1):
        assert _scan(L, algo=algo) == _capi.E_UNSUPPORTED
        assert "sq8" in err() and "tiled schedule only" in err() and f"algo={algo}" in err()
    assert _scan(L, algo=5) == _capi.E_INVALID and "algo=5" in err()
    # the uint8 pitch: a multiple of 16 elements, >= d
    assert _scan(L, d=100, row_stride=104) == _capi.E_INVALID and "row_stride=104" in err() and "multiple of 16" in err()
    assert _scan(L, d=100, row_stride=96) == _capi.E_INVALID and "row_stride=96" in err()
    assert _scan(L, d=1025, row_stride=1040) == _capi.E_UNSUPPORTED and "d=1025" in err()
    assert _scan(L, misalign=("corpus_sorted",)) == _capi.E_INVALID and "16-byte aligned" in err()
    for name in ("lo", "step"):
        assert _scan(L, null=(name,)) == _capi.E_INVALID and "null" in err() and "lo or step" in err(), name
        assert _scan(L, misalign=(name,)) == _capi.E_INVALID and "lo and step must be 16-byte aligned" in err(), name
    for name in ("corpus_sorted", "gid", "uniq_keys", "offsets", "queries", "qkeys", "nkeys", "out_dist", "out_idx", "out_ncand", "status",
                 "workspace"):
        assert _scan(L, null=(name,)) == _capi.E_INVALID and "null" in err(), name
    assert _scan(L, k=257) == _capi.E_UNSUPPORTED and "k=257" in err()
    assert _scan(L, phases=0) == _capi.E_INVALID and "phases=0" in err()
    assert _scan(L, ws_bytes=1024) == _capi.E_WORKSPACE and "workspace 1024" in err()
    # the typed calls keep answering INVALID to a fourth storage code
    keep, a = _buf()
    assert L.nlsh_gather_rows_typed(a, 0, 100, 100, a, 10, a, 3, 112, None, None, 0, a, None) == _capi.E_INVALID and "dst_storage=3" in err()


def _gather(L, src=F32, d=100, n=10, src_stride=None, dst_stride=112, null=(), misalign=()):
    keep, a = _buf()
    p = lambda name: None if name in null else a + (4 if name in ("sorted", "lo", "step") else 1) if name in misalign else a   # noqa: E731
    return L.nlsh_gather_rows_sq8(p("corpus"), src, d if src_stride is None else src_stride, d, p("perm"), n, p("sorted"), dst_stride,
                                  p("lo"), p("step"), None, None, 0, p("first_bad"), p("clamped_rows"), None)


def test_sq8_gather_refuses_on_the_host(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731

    def refused(text, **kw):
        assert _gather(L, **kw) == _capi.E_INVALID, kw
        assert text in err(), (text, err())

    refused("src_storage=3", src=3)
    refused("d=0", d=0)
    refused("d=1025", d=1025, dst_stride=2048)
    refused("n=-1", n=-1)
    refused("multiple of 16", dst_stride=104)
    refused("dst_stride=96", dst_stride=96)
    refused("src_stride=99", src_stride=99)
    refused("sorted must be 16-byte aligned", misalign=("sorted",))
    refused("lo and step must be 16-byte aligned", misalign=("lo",))
    refused("lo and step must be 16-byte aligned", misalign=("step",))
    refused("element size", src=F16, misalign=("corpus",))
    for name in ("corpus", "perm", "sorted"):
        refused("null", null=(name,))
    for name in ("lo", "step"):
        refused("lo / step is null", null=(name,))
    refused("first_bad", null=("first_bad",))                     # an encoding gather must be able to report
    # codes need no first_bad, and clamped_rows is optional (n = 0: nothing to launch, no pointer read)
    assert _gather(L, src=U8, n=0, null=("first_bad", "clamped_rows", "corpus", "perm", "sorted", "lo", "step")) == _capi.OK


def _train(L, storage=F32, d=100, n=1000, row_stride=None, quant_stride=112, null=(), misalign=(), ws_bytes=None):
    keep, a = _buf()
    need = L.nlsh_sq8_train_workspace(n, d) if n >= 0 and 1 <= d <= 1024 else 1 << 20
    p = lambda name: None if name in null else a + (4 if name == "workspace" else 1) if name in misalign else a   # noqa: E731
    return L.nlsh_sq8_train(p("rows"), storage, d if row_stride is None else row_stride, d, n, p("lo"), p("step"), quant_stride,
                            p("first_bad"), p("workspace"), need if ws_bytes is None else ws_bytes, None)


def test_sq8_train_refuses_on_the_host(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731

    def refused(text, rc=_capi.E_INVALID, **kw):
        assert _train(L, **kw) == rc, kw
        assert text in err(), (text, err())

    refused("storage=2", storage=U8)                              # codes have nothing to train on
    refused("storage=3", storage=3)
    refused("d=0", d=0)
    refused("d=1025", d=1025, quant_stride=2048)
    refused("n=-1", n=-1)
    refused("quant_stride=96", quant_stride=96)
    refused("row_stride=99", row_stride=99)
    refused("element size", misalign=("rows",))
    refused("16-byte aligned", misalign=("workspace",))
    for name in ("lo", "step", "first_bad", "rows", "workspace"):
        refused("null", null=(name,))
    refused("workspace 16", rc=_capi.E_WORKSPACE, ws_bytes=16)
    assert L.nlsh_sq8_train_workspace(-1, 8) == 0 and L.nlsh_sq8_train_workspace(8, 0) == 0 and L.nlsh_sq8_train_workspace(8, 1025) == 0
    assert L.nlsh_sq8_train_workspace(10 ** 9, 96) < (64 << 20)   # partials, not a copy


def _update(L, new_storage=F32, d=100, n_old=1000, nb_old=10, m_new=100, row_stride=112, stride_out=112, new_stride=None,
            ws_bytes=None, null=(), misalign=()):
    keep, a = _buf()
    need = L.nlsh_csr_update_workspace(n_old, nb_old, m_new) or (1 << 20)
    p = lambda name: None if name in null else a + 4 if name in misalign else a   # noqa: E731
    return L.nlsh_csr_update_sq8(
        p("corpus_sorted"), p("lo"), p("step"), row_stride, d, p("gid"), p("inv_norm"), p("uniq_keys"), p("offsets"), n_old, nb_old, None, n_old,
        p("rows_new"), new_storage, d if new_stride is None else new_stride, p("keys_new"), p("ids_new"), m_new,
        p("sorted_out"), stride_out, p("gid_out"), p("inv_norm_out"), p("src_out"), p("uniq_out"), p("offsets_out"), p("n_buckets_out"),
        p("first_bad"), p("clamped_rows"), p("workspace"), need if ws_bytes is None else ws_bytes, None)


def test_sq8_update_refuses_on_the_host(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731

    def refused(text, **kw):
        assert _update(L, **kw) == _capi.E_INVALID, kw
        assert text in err(), (text, err())

    refused("new_storage=-2", new_storage=-2)
    refused("multiple of 16", row_stride=104, stride_out=104)
    refused("row_stride=96", row_stride=96, stride_out=96)
    refused("lo and step are padded to ONE pitch", row_stride=112, stride_out=128)
    refused("new_stride=99", new_stride=99)
    refused("d=1025", d=1025, row_stride=2048, stride_out=2048, new_stride=2048)
    for name in ("corpus_sorted", "sorted_out", "workspace"):
        refused("16-byte aligned", misalign=(name,))
    for name in ("lo", "step"):
        refused("lo / step is null", null=(name,))
        refused("lo and step must be 16-byte aligned", misalign=(name,))
    for name in ("corpus_sorted", "gid", "uniq_keys", "offsets", "rows_new", "keys_new", "ids_new", "sorted_out", "gid_out", "src_out", "uniq_out",
                 "offsets_out", "n_buckets_out", "workspace"):
        refused(name, null=(name,))
    refused("first_bad", null=("first_bad",))                     # float rows into an sq8 index are encoded: they can be refused
    need = L.nlsh_csr_update_workspace(1000, 10, 100)
    refused("workspace_bytes", ws_bytes=need - 1)
    # codes need no first_bad, clamped_rows is optional: the call is stopped by the last check, the workspace size
    assert _update(L, new_storage=U8, null=("first_bad", "clamped_rows"), ws_bytes=0) == _capi.E_INVALID and "workspace_bytes" in err()


# ---------------------------------------------------------------------------------------------- the facade, without a device
def test_facade_refuses_before_touching_a_device():
    import torch
    from nlsh_amd import _capi
    from nlsh_amd.distributed import ShardedIndexer
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.multitable import MultiTableIndexer
    from nlsh_amd.pipeline import QueryPipeline
    host_corpus = torch.zeros(8, 4)
    lo, step = torch.zeros(4), torch.ones(4)
    with pytest.raises(ValueError, match="needs quantiser="):
        Indexer(None, torch.zeros(8, 4, dtype=torch.uint8), None, metric="l2", storage="sq8")
    for bad, text in (((lo, step, step), "pair"), (lo, "pair"), ((lo[:3], step), r"shape \(4,\)"), ((lo, step.reshape(1, 4)), r"shape \(4,\)"),
                      ((lo.double(), step), "float32"), ((lo, step.half()), "float32"), ((lo, torch.tensor([1.0, 0.0, 1.0, 1.0])), "step must be > 0"),
                      ((lo, -step), "step must be > 0"), ((lo, torch.tensor([1.0, float("nan"), 1.0, 1.0])), "finite"),
                      ((torch.tensor([0.0, float("inf"), 0.0, 0.0]), step), "finite")):
        with pytest.raises(ValueError, match=text):
            Indexer(None, host_corpus, None, metric="l2", storage="sq8", quantiser=bad)
    for storage in (None, "float32", "float16", "uint8"):
        with pytest.raises(ValueError, match="quantiser= belongs to storage='sq8'"):
            Indexer(None, host_corpus, None, metric="l2", storage=storage, quantiser=(lo, step))
    with pytest.raises(ValueError, match="quantiser= belongs to storage='sq8'"):
        MultiTableIndexer([object()], host_corpus, None, metric="l2", storage="uint8", quantiser=(lo, step))
    for algo in ("query", "bucket"):
        with pytest.raises(ValueError, match="tiled schedule only"):
            Indexer(None, host_corpus, None, metric="l2", storage="sq8", algo=algo)
    # a valid request reaches the corpus check: there is still no CPU path
    for q in (None, (lo, step), (lo.numpy(), step.numpy())):
        with pytest.raises(_capi.NlshHipError, match="no CPU path"):
            Indexer(None, host_corpus, None, metric="l2", storage="sq8", algo="tiled", quantiser=q)
    ix = Indexer.__new__(Indexer)
    ix.storage = "sq8"
    assert ix.compressed and ix.choose_algo(1, 1) == _capi.SCAN_BUCKET_TILED and ix.choose_algo(10 ** 4, 10) == _capi.SCAN_BUCKET_TILED
    assert not ix._fuses(None, 10, _capi.SCAN_BUCKET_TILED) and not ix._fuses_ranked(None, 10, _capi.SCAN_BUCKET_TILED, ranked=True)
    with pytest.raises(NotImplementedError, match="storage='sq8'"):
        QueryPipeline(ix, host_corpus)
    with pytest.raises(NotImplementedError, match="storage='sq8'"):
        ShardedIndexer(None, host_corpus, None, id_base=0, storage="sq8")
    for call in (lambda: ix.range_query(host_corpus, 1.0), lambda: ix.range_tensors(host_corpus, 1.0),
                 lambda: ix.range_scan_tensors(host_corpus, None, None, 1.0), lambda: ix.range_query_with_keys(host_corpus, [[1]] * 8, 1.0)):
        with pytest.raises(NotImplementedError, match="storage='sq8'"):
            call()
    plain = Indexer.__new__(Indexer)
    plain.storage = "uint8"
    with pytest.raises(AttributeError, match="no quantiser"):
        plain.quantiser


# ---------------------------------------------------------------------------------------------- the compiled kernels
def test_affine_scan_kernels_are_clean():
    """bscana_kernel = the tiled task body with the decode where the tile is written and the filter's bit in its epilogue: the same
    hand-placed scalar loads, so the same lint; 6 instantiations (3 metrics x narrow / wide k), no scratch, no VGPR spill, the 20 KB tile,
    and the occupancy bound the filtered kernels are held to."""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    if not (os.path.exists(isa_lint.HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not installed")
    rep = isa_lint.lint("scan_bucket_affine.hip", "bscana_kernel")
    assert len(rep) == 6, sorted(rep)
    for name, r in rep.items():
        res = r["resources"]
        assert r["scalar_loads"] > 100, name
        assert r["violations"] == [], (name, r["violations"][:5])
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (name, res)
        assert not [x for x in r["hot_loop_spills"] if x.startswith("v_writelane")], (name, r["hot_loop_spills"][:5])
        assert res["Occupancy"] >= 6 and res["VGPRs"] <= 80 and res["LDS Size"] <= 20480, (name, res)
