"""Float16 / uint8 corpus storage, the parts that need no device: the three typed exports against the header and the binding, every
host-side refusal of the three calls (nothing is launched and no pointer is read before the checks pass), the facade's refusals, and the
conversion rule restated in numpy -- `representable` / `convert` / `first_bad_row` below are the reference of the GPU conversion tests
(tests/test_gpu_corpus_storage.py imports them)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, U8 = 0, 1, 2


# ---------------------------------------------------------------------------------------------- the conversion rule
def representable(x, storage):
    """Per element: does float32 `x` survive the conversion to `storage`?  float16: everything but a finite value that rounds (to
    nearest even) to an infinity; uint8: integers in [0, 255] only (a NaN is none)."""
    x = np.asarray(x, np.float32)
    if storage == "float16":
        with np.errstate(over="ignore"):
            h = x.astype(np.float16)
        return ~(np.isinf(h) & np.isfinite(x))
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (x <= 255) & (x == np.trunc(x))


def convert(x, storage):
    """Representable float32 values as `storage` holds them (numpy's float16 cast rounds to nearest even, as `torch.Tensor.half()`)."""
    x = np.asarray(x, np.float32)
    assert representable(x, storage).all()
    return x.astype(np.float16) if storage == "float16" else np.abs(x).astype(np.uint8)


def first_bad_row(rows, storage):
    bad = ~representable(rows, storage).all(axis=1)
    return int(np.argmax(bad)) if bad.any() else -1


def test_float16_rule_is_round_to_nearest_even_and_refuses_only_overflow():
    # ties between two float16 neighbours go to the even mantissa: 1 + 2^-11 -> 1, 1 + 3 * 2^-11 -> 1 + 2^-9
    ties = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2048 + 1, 2048 + 3, -(1 + 2.0 ** -11)], np.float32)
    assert convert(ties, "float16").tolist() == [1.0, 1 + 2.0 ** -9, 2048.0, 2052.0, -1.0]
    # just above / below a tie: nearest
    assert convert(np.array([1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -11 - 2.0 ** -20], np.float32), "float16").tolist() == [1 + 2.0 ** -10, 1.0]
    # subnormals: 2^-24 is the smallest, 2^-25 is a tie between 0 and 2^-24 -> 0 (even), 1.5 * 2^-24 is a tie -> 2^-23
    sub = convert(np.array([2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, -(2.0 ** -24)], np.float32), "float16")
    assert sub.view(np.uint16).tolist() == [0x0001, 0x0000, 0x0002, 0x8001]
    # the overflow boundary: 65504 is the largest finite float16, 65520 is the tie between it and 2^16 -> infinity: refused
    edge = np.array([65504, -65504, 65519.996, 65520, -65520, 1e30, np.inf, -np.inf, np.nan, -0.0], np.float32)
    assert representable(edge, "float16").tolist() == [True, True, True, False, False, False, True, True, True, True]
    assert convert(np.array([-0.0], np.float32), "float16").view(np.uint16).tolist() == [0x8000]      # the sign of zero is kept


def test_uint8_rule_takes_integers_in_range_only():
    x = np.array([0, 1, 255, -0.0, 0.5, 254.999, 256, -1, 1e9, np.nan, np.inf, -np.inf, 2.0 ** -30, 128], np.float32)
    assert representable(x, "uint8").tolist() == [True, True, True, True, False, False, False, False, False, False, False, False, False, True]
    assert convert(np.array([0, 1, 255, -0.0, 128], np.float32), "uint8").tolist() == [0, 1, 255, 0, 128]
    rows = np.zeros((5, 3), np.float32)
    assert first_bad_row(rows, "uint8") == -1
    rows[3, 1], rows[4, 0] = 0.25, 300
    assert first_bad_row(rows, "uint8") == 3


# ---------------------------------------------------------------------------------------------- the C ABI, host side
@pytest.fixture(scope="module")
def L():
    from nlsh_amd import _capi
    return _capi.lib()


TYPED = ("nlsh_scan_topk_cells_phase_typed", "nlsh_gather_rows_typed", "nlsh_csr_update_typed")


def test_typed_exports_exist_and_header_binding_and_library_agree(L):
    from nlsh_amd import _capi
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    for sym in TYPED:
        assert sym in _capi.SYMBOLS and hasattr(L, sym)
        decl = re.search(r"int %s\((.*?)\);" % sym, header, re.S)
        assert decl, sym
        assert len(getattr(L, sym).argtypes) == len(decl.group(1).split(",")), sym
    # a typed call is its untyped twin plus the storage codes (and first_bad)
    assert len(L.nlsh_scan_topk_cells_phase_typed.argtypes) == len(L.nlsh_scan_topk_cells_phase.argtypes) + 1
    assert len(L.nlsh_gather_rows_typed.argtypes) == len(L.nlsh_gather_rows.argtypes) + 3
    assert len(L.nlsh_csr_update_typed.argtypes) == len(L.nlsh_csr_update.argtypes) + 3
    for name, val in (("F32", 0), ("F16", 1), ("U8", 2)):
        assert int(re.search(r"#define NLSH_STORE_%s (\d+)" % name, header).group(1)) == val == getattr(_capi, "STORE_" + name)


def test_the_abi_version_and_the_step_descriptor_did_not_move(L):
    from nlsh_amd import _capi
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    assert int(re.search(r"#define NLSH_ABI_VERSION (\d+)", header).group(1)) == 4 and L.nlsh_abi_version() == 4
    assert "storage" not in [f[0] for f in _capi.StepDesc._fields_]          # the step / batch / graph entry points stay float32


def _buf():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 255) & ~255


def _scan(L, storage=F16, algo=2, row_stride=128, d=128, k=10, null=(), misalign=(), ws_bytes=None, Q=4, P=2, max_tasks=64, nb=3, phases=7):
    """nlsh_scan_topk_cells_phase_typed with pointers into a small host buffer: every call here must be refused before any is used."""
    keep, a = _buf()
    need = L.nlsh_scan_workspace(Q, P, k, max_tasks, nb, d)
    p = lambda name: None if name in null else a + 4 if name in misalign else a   # noqa: E731
    return L.nlsh_scan_topk_cells_phase_typed(
        p("corpus_sorted"), storage, row_stride, d, p("gid"), p("uniq_keys"), p("offsets"), None, nb, None, None, 0, p("inv_norm"),
        p("queries"), d, Q, p("qkeys"), p("nkeys"), P, k, 0, algo, 0, p("out_dist"), p("out_idx"), None, p("out_ncand"), p("status"),
        p("workspace"), need if ws_bytes is None else ws_bytes, max_tasks, None, None, None, phases)


def test_typed_scan_refuses_on_the_host(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731
    for storage in (-1, 3, 17):
        assert _scan(L, storage=storage) == _capi.E_INVALID and f"storage={storage}" in err()
    # the two other schedules cannot read typed rows: UNSUPPORTED, with the reason
    for storage, name in ((F16, "float16"), (U8, "uint8")):
        for algo in (0, 1):
            assert _scan(L, storage=storage, algo=algo, row_stride=128) == _capi.E_UNSUPPORTED
            assert name in err() and "tiled schedule only" in err() and f"algo={algo}" in err()
    assert _scan(L, algo=5) == _capi.E_INVALID and "algo=5" in err()
    # the pitch is a multiple of 16 bytes: 8 float16 / 16 uint8 elements
    assert _scan(L, storage=F16, d=100, row_stride=100) == _capi.E_INVALID and "row_stride=100" in err() and "multiple of 8" in err()
    assert _scan(L, storage=U8, d=100, row_stride=104) == _capi.E_INVALID and "row_stride=104" in err() and "multiple of 16" in err()
    assert _scan(L, storage=U8, d=100, row_stride=96) == _capi.E_INVALID and "row_stride=96" in err()       # < d
    assert _scan(L, misalign=("corpus_sorted",)) == _capi.E_INVALID and "16-byte aligned" in err()
    for name in ("corpus_sorted", "gid", "uniq_keys", "offsets", "queries", "qkeys", "nkeys", "out_dist", "out_idx", "out_ncand", "status",
                 "workspace"):
        assert _scan(L, null=(name,)) == _capi.E_INVALID and "null" in err(), name
    assert _scan(L, k=257) == _capi.E_UNSUPPORTED and "k=257" in err()
    assert _scan(L, phases=0) == _capi.E_INVALID and "phases=0" in err()
    # a short workspace: refused by size, before the first launch
    assert _scan(L, ws_bytes=1024) == _capi.E_WORKSPACE and "workspace 1024" in err()


def _gather(L, src=F32, dst=F16, d=100, n=10, src_stride=None, dst_stride=104, null=(), misalign=()):
    keep, a = _buf()
    p = lambda name: None if name in null else a + (4 if name == "sorted" else 1) if name in misalign else a   # noqa: E731
    return L.nlsh_gather_rows_typed(p("corpus"), src, d if src_stride is None else src_stride, d, p("perm"), n, p("sorted"), dst, dst_stride,
                                    None, None, 0, p("first_bad"), None)


def test_typed_gather_refuses_on_the_host(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731

    def refused(text, **kw):
        assert _gather(L, **kw) == _capi.E_INVALID, kw
        assert text in err(), (text, err())

    refused("src_storage=3", src=3)
    refused("dst_storage=-1", dst=-1)
    refused("d=0", d=0)
    refused("d=1025", d=1025, dst_stride=2048)
    refused("n=-1", n=-1)
    refused("dst_stride=100", dst=F16, dst_stride=100)            # 200 bytes: not a pitch of 16-byte units
    refused("multiple of 16", dst=U8, dst_stride=104)
    refused("multiple of 4", dst=F32, src=F16, dst_stride=102)
    refused("dst_stride=96", dst=U8, dst_stride=96)               # < d
    refused("src_stride=99", src_stride=99)
    refused("16-byte aligned", misalign=("sorted",))
    refused("element size", src=F16, dst=F16, misalign=("corpus",))
    for name in ("corpus", "perm", "sorted"):
        refused("null", null=(name,))
    refused("first_bad", null=("first_bad",))                     # a converting gather must be able to report
    # ... and the last check passed is the last host check: a same-storage gather needs no first_bad (n = 0: nothing to launch)
    assert _gather(L, src=U8, dst=U8, n=0, null=("first_bad", "corpus", "perm", "sorted")) == _capi.OK


def _update(L, storage=F16, new_storage=F32, d=100, n_old=1000, nb_old=10, m_new=100, row_stride=104, stride_out=104, new_stride=None,
            ws_bytes=None, null=(), misalign=()):
    keep, a = _buf()
    need = L.nlsh_csr_update_workspace(n_old, nb_old, m_new) or (1 << 20)
    p = lambda name: None if name in null else a + 4 if name in misalign else a   # noqa: E731
    return L.nlsh_csr_update_typed(
        p("corpus_sorted"), storage, row_stride, d, p("gid"), p("inv_norm"), p("uniq_keys"), p("offsets"), n_old, nb_old, None, n_old,
        p("rows_new"), new_storage, d if new_stride is None else new_stride, p("keys_new"), p("ids_new"), m_new,
        p("sorted_out"), stride_out, p("gid_out"), p("inv_norm_out"), p("src_out"), p("uniq_out"), p("offsets_out"), p("n_buckets_out"),
        p("first_bad"), p("workspace"), need if ws_bytes is None else ws_bytes, None)


def test_typed_update_refuses_on_the_host(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731

    def refused(text, **kw):
        assert _update(L, **kw) == _capi.E_INVALID, kw
        assert text in err(), (text, err())

    refused("storage=3", storage=3)
    refused("new_storage=-2", new_storage=-2)
    refused("row_stride=100", row_stride=100)                     # float16: 8 elements per 16 bytes
    refused("stride_out=100", stride_out=100)
    refused("multiple of 16", storage=U8, row_stride=104, stride_out=112)
    refused("stride_out=104", storage=U8, row_stride=112, stride_out=104)
    refused("row_stride=96", row_stride=96)                       # < d
    refused("new_stride=99", new_stride=99)
    refused("d=1025", d=1025, row_stride=2048, stride_out=2048, new_stride=2048)
    for name in ("corpus_sorted", "sorted_out", "workspace"):
        refused("16-byte aligned", misalign=(name,))
    for name in ("corpus_sorted", "gid", "uniq_keys", "offsets", "rows_new", "keys_new", "ids_new", "sorted_out", "gid_out", "src_out", "uniq_out",
                 "offsets_out", "n_buckets_out", "workspace"):
        refused(name, null=(name,))
    refused("first_bad", null=("first_bad",))                     # float32 rows into a float16 index are converted: they can fail
    need = L.nlsh_csr_update_workspace(1000, 10, 100)
    refused("workspace_bytes", ws_bytes=need - 1)
    # rows of the index's own storage need no first_bad: the call passes that check and is stopped by the last one, the workspace size
    assert _update(L, storage=U8, new_storage=U8, row_stride=112, stride_out=112, null=("first_bad",), ws_bytes=0) == _capi.E_INVALID
    assert "workspace_bytes" in err()


# ---------------------------------------------------------------------------------------------- the facade, without a device
def test_facade_refuses_before_touching_a_device():
    import torch
    from nlsh_amd import _capi
    from nlsh_amd.distributed import ShardedIndexer
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.pipeline import QueryPipeline
    host_corpus = torch.zeros(8, 4)
    for bad in ("int8", "fp16", "bfloat16", 16, ""):
        with pytest.raises(ValueError, match="storage must be"):
            Indexer(None, host_corpus, None, metric="l2", storage=bad)
    for storage in ("float16", "uint8"):
        for algo in ("query", "bucket"):
            with pytest.raises(ValueError, match="tiled schedule only"):
                Indexer(None, host_corpus, None, metric="l2", storage=storage, algo=algo)
        # a valid request reaches the corpus check: there is still no CPU path
        with pytest.raises(_capi.NlshHipError, match="no CPU path"):
            Indexer(None, host_corpus, None, metric="l2", storage=storage, algo="tiled")
        ix = Indexer.__new__(Indexer)
        ix.storage = storage
        assert ix.compressed and ix.choose_algo(1, 1) == _capi.SCAN_BUCKET_TILED and ix.choose_algo(10 ** 4, 10) == _capi.SCAN_BUCKET_TILED
        assert not ix._fuses(None, 10, _capi.SCAN_BUCKET_TILED) and not ix._fuses_ranked(None, 10, _capi.SCAN_BUCKET_TILED, ranked=True)
        with pytest.raises(NotImplementedError, match="storage="):
            QueryPipeline(ix, host_corpus)
        with pytest.raises(NotImplementedError, match="storage="):
            ShardedIndexer(None, host_corpus, None, id_base=0, storage=storage)
    plain = Indexer.__new__(Indexer)
    assert plain.storage == "float32" and not plain.compressed

