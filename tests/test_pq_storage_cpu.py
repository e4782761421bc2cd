"""storage="pq" without a device: the numpy statement of the rule (tests/pq_ref.py) against a float64 brute force, the exports, and every
refusal of the C entry points and of the facade, each before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import pq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PQ = ("nlsh_pq_encode", "nlsh_pq_decode_rows", "nlsh_pq_inv_norm", "nlsh_scan_topk_cells_phase_pq")


# ---------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("d, dsub", [(1, 4), (12, 8), (16, 4), (100, 16), (33, 8)])
def test_the_numpy_rule_is_the_float64_argmin_on_integer_data_with_real_ties(d, dsub):
    """Integer-valued rows and centroids below 2^10: every float32 subtract, square and partial sum is exact, so the float32 rule and the
    float64 brute force see the same scores, equal scores are real ties, and both must name the lowest index."""
    rng = np.random.default_rng(d * 100 + dsub)
    M = pq_ref.n_sub(d, dsub)
    C = rng.integers(-40, 41, size=(M, 256, dsub)).astype(np.float32)
    C[:, 7] = C[:, 3]
    C[:, 128:] = C[:, :128]                                          # every centroid twice: each minimum is at least a two-way tie
    C = pq_ref.zero_tail(C, d)
    X = rng.integers(-60, 61, size=(500, d)).astype(np.float32)
    X[:128, :min(d, dsub)] = C[0, 128:, :min(d, dsub)]               # rows that ARE a duplicated centroid: score 0 at two indices
    codes, bad = pq_ref.pq_encode(X, C, d)
    assert bad == -1 and codes.dtype == np.uint8 and codes.shape == (500, M)
    assert np.array_equal(codes, pq_ref.brute_f64(X, C, d))
    assert int(codes.max()) < 128, "a tie never goes to the later copy"
    R = pq_ref.pq_decode(codes, C, d)
    assert R.shape == (500, d) and R.dtype == np.float32
    for j in (0, d // 2, d - 1):
        assert np.array_equal(R[:, j], C[j // dsub, codes[:, j // dsub], j % dsub])
    # the decoded row is at least as near as any other centroid choice, sub-vector by sub-vector
    assert np.array_equal(pq_ref.pq_encode(R, C, d)[0], codes)


def test_the_rule_skips_columns_beyond_d_refuses_non_finite_rows_and_survives_overflow():
    d, dsub = 5, 4
    C = np.zeros((2, 256, 4), np.float32)
    C[1, :, 0] = np.arange(256)
    C[1, :, 1:] = 1e30                                               # beyond d: must not enter a score (zero_tail clears them anyway)
    X = np.zeros((4, d), np.float32)
    X[:, 4] = [3.2, 250.6, -9.0, 1000.0]
    codes, bad = pq_ref.pq_encode(X, C, d)
    assert bad == -1 and codes[:, 1].tolist() == [3, 251, 0, 255]
    assert pq_ref.zero_tail(C, d)[1, :, 1:].max() == 0.0
    X[2, 1], X[1, 0] = np.inf, np.nan
    assert pq_ref.pq_encode(X, C, d)[1] == 1
    big = np.full((1, 256, 4), 3e38, np.float32)
    big[0, 200] = 2.9e38                                             # every difference overflows, every score is +inf: all tie, index 0 stands
    assert pq_ref.pq_encode(np.full((2, 4), -3e38, np.float32), big, 4)[0].tolist() == [[0], [0]]
    big[0, 7, :] = -3e38                                             # ... but one finite score wins
    assert pq_ref.pq_encode(np.full((2, 4), -3e38, np.float32), big, 4)[0].tolist() == [[7], [7]]


# ---------------------------------------------------------------------------------------------- the C ABI, host side
@pytest.fixture(scope="module")
def L():
    from nlsh_amd import _capi
    return _capi.lib()


def test_pq_exports_exist_and_header_binding_and_library_agree(L):
    from nlsh_amd import _capi
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    for sym in PQ:
        assert sym in _capi.SYMBOLS and hasattr(L, sym)
        decl = re.search(r"(?:int|size_t) %s\((.*?)\);" % sym, header, re.S)
        assert decl, sym
        assert len(getattr(L, sym).argtypes) == len(decl.group(1).split(",")), sym
    # the pq scan is the sq8 scan with (codebook, dsub, code_pitch) where (lo, step) stand
    assert len(L.nlsh_scan_topk_cells_phase_pq.argtypes) == len(L.nlsh_scan_topk_cells_phase_sq8.argtypes) + 1
    # the ABI did not move, and pq is no storage code of the typed calls
    assert int(re.search(r"#define NLSH_ABI_VERSION (\d+)", header).group(1)) == 4 and L.nlsh_abi_version() == 4
    assert not re.search(r"#define NLSH_STORE_\w+ [34]", header)


def _buf():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 255) & ~255


def _scan(L, algo=2, d=128, dsub=8, pitch=16, row_stride=None, k=10, null=(), misalign=(), ws_bytes=None, Q=4, P=2, max_tasks=64, nb=3, phases=7):
    """nlsh_scan_topk_cells_phase_pq with pointers into a small host buffer: every call here must be refused before any is used."""
    keep, a = _buf()
    need = L.nlsh_scan_workspace(Q, P, k, max_tasks, nb, d)
    p = lambda name: None if name in null else a + 4 if name in misalign else a   # noqa: E731
    M = (d + dsub - 1) // dsub if dsub > 0 else 1
    return L.nlsh_scan_topk_cells_phase_pq(
        p("corpus_sorted"), p("codebook"), dsub, pitch, M * dsub if row_stride is None else row_stride, d, p("gid"), p("uniq_keys"), p("offsets"),
        None, nb, None, None, 0, p("inv_norm"), p("queries"), d, Q, p("qkeys"), p("nkeys"), P, k, 0, algo, 0, p("out_dist"), p("out_idx"), None,
        p("out_ncand"), p("status"), p("workspace"), need if ws_bytes is None else ws_bytes, max_tasks, None, None, None, phases, None)


def test_pq_scan_refuses_on_the_host(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731
    for algo in (0, 1):
        assert _scan(L, algo=algo) == _capi.E_UNSUPPORTED
        assert "pq" in err() and "tiled schedule only" in err() and f"algo={algo}" in err()
    assert _scan(L, algo=5) == _capi.E_INVALID and "algo=5" in err()
    for dsub in (0, 2, 5, 12, 32, -8):
        assert _scan(L, dsub=dsub) == _capi.E_INVALID and f"dsub={dsub}" in err(), dsub
    assert _scan(L, null=("codebook",)) == _capi.E_INVALID and "codebook" in err() and "null" in err()
    assert _scan(L, misalign=("codebook",)) == _capi.E_INVALID and "codebook" in err() and "16-byte aligned" in err()
    # the code pitch: a multiple of 16 bytes, >= M; row_stride: the decoded width
    assert _scan(L, d=100, dsub=4, pitch=16) == _capi.E_INVALID and "code_pitch=16" in err() and "M=25" in err()
    assert _scan(L, d=100, dsub=8, pitch=24) == _capi.E_INVALID and "code_pitch=24" in err() and "multiple of 16" in err()
    assert _scan(L, d=100, dsub=8, row_stride=100) == _capi.E_INVALID and "row_stride=100" in err() and "104" in err()
    assert _scan(L, misalign=("corpus_sorted",)) == _capi.E_INVALID and "16-byte aligned" in err()
    assert _scan(L, d=1025, dsub=16, pitch=80) == _capi.E_UNSUPPORTED and "d=1025" in err()
    for name in ("corpus_sorted", "gid", "uniq_keys", "offsets", "queries", "qkeys", "nkeys", "out_dist", "out_idx", "out_ncand", "status",
                 "workspace"):
        assert _scan(L, null=(name,)) == _capi.E_INVALID and "null" in err(), name
    assert _scan(L, k=257) == _capi.E_UNSUPPORTED and "k=257" in err()
    assert _scan(L, phases=0) == _capi.E_INVALID and "phases=0" in err()
    assert _scan(L, phases=8) == _capi.E_INVALID and "phases=8" in err()        # the plan-rest bit is not the C ABI's
    assert _scan(L, ws_bytes=1024) == _capi.E_WORKSPACE and "workspace 1024" in err()


def test_pq_row_calls_refuse_on_the_host(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731
    keep, a = _buf()
    F32, F16, U8 = _capi.STORE_F32, _capi.STORE_F16, _capi.STORE_U8

    def encode(rows=a, storage=F32, row_stride=100, d=100, n=10, cb=a, dsub=8, codes=a, pitch=13, bad=a):
        return L.nlsh_pq_encode(rows, storage, row_stride, d, n, cb, dsub, codes, pitch, bad, None)

    assert encode(storage=U8) == _capi.E_INVALID and "storage=2" in err()
    assert encode(storage=7) == _capi.E_INVALID
    for dsub in (0, 3, 32):
        assert encode(dsub=dsub) == _capi.E_INVALID and f"dsub={dsub}" in err()
    assert encode(cb=None) == _capi.E_INVALID and "codebook" in err()
    assert encode(cb=a + 4) == _capi.E_INVALID and "codebook" in err()
    assert encode(d=0) == _capi.E_INVALID and encode(d=1025) == _capi.E_INVALID and encode(n=-1) == _capi.E_INVALID
    assert encode(rows=None) == _capi.E_INVALID and encode(codes=None) == _capi.E_INVALID and encode(bad=None) == _capi.E_INVALID
    assert encode(row_stride=99) == _capi.E_INVALID and "row_stride=99" in err()
    assert encode(pitch=12) == _capi.E_INVALID and "code_pitch=12" in err() and "M=13" in err()
    assert encode(rows=a + 2) == _capi.E_INVALID and "element size" in err()
    assert encode(rows=a + 1, storage=F16) == _capi.E_INVALID

    def decode(codes=a, pitch=16, n=10, cb=a, dsub=8, d=100, out=a, out_stride=100):
        return L.nlsh_pq_decode_rows(codes, pitch, n, cb, dsub, d, out, out_stride, None)

    assert decode(dsub=6) == _capi.E_INVALID and decode(cb=None) == _capi.E_INVALID and decode(codes=None) == _capi.E_INVALID
    assert decode(out=None) == _capi.E_INVALID and decode(out=a + 2) == _capi.E_INVALID
    assert decode(out_stride=99) == _capi.E_INVALID and "out_stride=99" in err()
    assert decode(pitch=12) == _capi.E_INVALID
    assert decode(n=0, codes=None, out=None) == _capi.OK                         # nothing to do, nothing looked at

    def inv(codes=a, pitch=16, n=10, cb=a, dsub=8, d=100, out=a):
        return L.nlsh_pq_inv_norm(codes, pitch, n, cb, dsub, d, out, None)

    assert inv(dsub=1) == _capi.E_INVALID and inv(cb=a + 8) == _capi.E_INVALID and inv(codes=None) == _capi.E_INVALID
    assert inv(out=None) == _capi.E_INVALID and inv(pitch=3) == _capi.E_INVALID
    assert inv(n=0, codes=None, out=None) == _capi.OK
    # the typed calls keep answering INVALID to a storage code past NLSH_STORE_U8
    assert L.nlsh_gather_rows_typed(a, 0, 100, 100, a, 10, a, 4, 112, None, None, 0, a, None) == _capi.E_INVALID and "dst_storage=4" in err()


# ---------------------------------------------------------------------------------------------- the facade, without a device
def test_facade_refuses_before_touching_a_device():
    import torch
    from nlsh_amd import _capi
    from nlsh_amd.distributed import ShardedIndexer
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.multitable import MultiTableIndexer
    from nlsh_amd.pipeline import QueryPipeline
    from nlsh_amd.training import pq_train
    host_corpus = torch.zeros(8, 12)
    good = torch.zeros(2, 256, 8)
    for dsub in (0, 2, 6, 32, 8.5, "8", True):
        with pytest.raises(ValueError, match="pq_dsub must be one of"):
            Indexer(None, host_corpus, None, metric="l2", storage="pq", pq_dsub=dsub)
        with pytest.raises(ValueError, match="dsub must be one of"):
            pq_train(host_corpus, dsub)
    nan = good.clone()
    nan[1, 5, 2] = float("nan")
    inf = good.clone()
    inf[0, 0, 0] = float("-inf")
    for bad, text in ((torch.zeros(2, 256, 4), r"shape \(2, 256, 8\)"), (torch.zeros(3, 256, 8), r"shape \(2, 256, 8\)"),
                      (torch.zeros(2, 255, 8), r"shape \(2, 256, 8\)"), (torch.zeros(2, 256 * 8), r"shape \(2, 256, 8\)"),
                      (good.double(), "float32"), (good.half(), "float32"), (nan, "finite"), (inf, "finite"),
                      ((torch.zeros(12), torch.ones(12)), "must be a codebook")):
        with pytest.raises(ValueError, match=text):
            Indexer(None, host_corpus, None, metric="l2", storage="pq", quantiser=bad)
    with pytest.raises(ValueError, match=r"shape \(3, 256, 4\)"):
        Indexer(None, host_corpus, None, metric="l2", storage="pq", pq_dsub=4, quantiser=good)
    with pytest.raises(ValueError, match="needs quantiser=codebook"):
        Indexer(None, torch.zeros(8, 2, dtype=torch.uint8), None, metric="l2", storage="pq")
    with pytest.raises(ValueError, match="pq_dim=17"):
        Indexer(None, torch.zeros(8, 2, dtype=torch.uint8), None, metric="l2", storage="pq", quantiser=good, pq_dim=17)
    for storage in (None, "float32", "float16", "uint8"):
        with pytest.raises(ValueError, match="quantiser= belongs to storage="):
            Indexer(None, host_corpus, None, metric="l2", storage=storage, quantiser=good)
        with pytest.raises(ValueError, match="pq_dsub= / pq_dim= belong to storage='pq'"):
            Indexer(None, host_corpus, None, metric="l2", storage=storage, pq_dsub=8)
        with pytest.raises(ValueError, match="pq_dsub= / pq_dim= belong to storage='pq'"):
            MultiTableIndexer([object()], host_corpus, None, metric="l2", storage=storage, pq_dsub=8)
    with pytest.raises(ValueError, match="pq_dsub= / pq_dim= belong to storage='pq'"):
        Indexer(None, host_corpus, None, metric="l2", storage="sq8", pq_dsub=8)
    with pytest.raises(ValueError, match="pair"):
        Indexer(None, host_corpus, None, metric="l2", storage="sq8", quantiser=good)
    for algo in ("query", "bucket"):
        with pytest.raises(ValueError, match="tiled schedule only"):
            Indexer(None, host_corpus, None, metric="l2", storage="pq", algo=algo)
    with pytest.raises(NotImplementedError, match="storage='pq'"):
        Indexer(None, host_corpus, None, metric="l2", storage="pq", tags=torch.zeros(8, dtype=torch.int64))
    # a valid request reaches the corpus check: there is still no CPU path
    for q in (None, good, good.numpy()):
        with pytest.raises(_capi.NlshHipError, match="no CPU path"):
            Indexer(None, host_corpus, None, metric="l2", storage="pq", algo="tiled", quantiser=q)
    ix = Indexer.__new__(Indexer)
    ix.storage = "pq"
    assert ix.compressed and ix.choose_algo(1, 1) == _capi.SCAN_BUCKET_TILED and ix.choose_algo(10 ** 4, 10) == _capi.SCAN_BUCKET_TILED
    assert not ix._fuses(None, 10, _capi.SCAN_BUCKET_TILED) and not ix._fuses_ranked(None, 10, _capi.SCAN_BUCKET_TILED, ranked=True)
    with pytest.raises(NotImplementedError, match="storage='pq'"):
        QueryPipeline(ix, host_corpus)
    with pytest.raises(NotImplementedError, match="storage='pq'"):
        ShardedIndexer(None, host_corpus, None, id_base=0, storage="pq")
    for call in (lambda: ix.range_query(host_corpus, 1.0), lambda: ix.range_tensors(host_corpus, 1.0),
                 lambda: ix.range_scan_tensors(host_corpus, None, None, 1.0), lambda: ix.range_query_with_keys(host_corpus, [[1]] * 8, 1.0)):
        with pytest.raises(NotImplementedError, match="storage='pq'"):
            call()
    for call in (lambda: ix.query_tensors(host_corpus, tag_mask=1), lambda: ix.scan_tensors(host_corpus, None, None, tag_mask=1),
                 lambda: ix.query(host_corpus, tag_mask=1), lambda: ix.query_with_keys(host_corpus, [[1]] * 8, tag_mask=1)):
        with pytest.raises(NotImplementedError, match="storage='pq'"):
            call()
    plain = Indexer.__new__(Indexer)
    plain.storage = "uint8"
    with pytest.raises(AttributeError, match="no codebook"):
        plain.codebook
    # the tail of a given codebook is zeroed on intake, on a copy
    from nlsh_amd.indexer import checked_codebook
    ones = torch.ones(2, 256, 8)
    held = checked_codebook(ones, 12, 8)
    assert bool((held[1, :, 4:] == 0).all()) and bool((held[1, :, :4] == 1).all()) and bool((held[0] == 1).all()) and bool((ones == 1).all())
