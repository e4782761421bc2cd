"""ctypes binding of the C ABI in include/nlsh_hip.h (lib/libnlsh_hip.so, built for gfx950).

The product path has NO fallback: if the library is missing or a call fails, an exception is
raised (`NlshHipError`).  Nothing here imports or calls the CPU oracle.
"""
import ctypes
import os
import subprocess

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("NLSH_HIP_LIB") or os.path.join(_PKG, "lib", "libnlsh_hip.so")   # override: diagnostic builds only
CSRC = os.path.join(_PKG, "csrc")

OK, E_INVALID, E_UNSUPPORTED, E_HIP, E_WORKSPACE = 0, -1, -2, -3, -4
ACT_SIGMOID, ACT_TANH = 0, 1
KEY_REF_INT16, KEY_FULL = 0, 1
METRIC_L2_EPS, METRIC_COSINE, METRIC_L2_EPS_FOLDED = 0, 1, 2
SCAN_QUERY_MAJOR, SCAN_BUCKET_MAJOR, SCAN_BUCKET_TILED = 0, 1, 2
STORE_F32, STORE_F16, STORE_U8 = 0, 1, 2   # NLSH_STORE_*: element type of a bucket-sorted corpus copy (the *_typed entry points)
TAG_ANY, TAG_ALL, TAG_EQ = 0, 1, 2         # NLSH_TAG_*: match mode of a tagged scan call (row tags against query masks)
MAX_LAYERS, MAX_HASH_BITS, MAX_PROBES, MAX_K, MAX_DIM, MAX_WIDTH = 8, 32, 64, 64, 1024, 632
MAX_K_TILED = 256  # k of the tiled schedule and of nlsh_merge_topk (NLSH_MAX_K_TILED); MAX_K is what every schedule takes
MAX_TABLES = 16    # lists per query of nlsh_merge_topk_unique = hash tables of a MultiTableIndexer (NLSH_MAX_TABLES)
PHASE_PLAN, PHASE_SCAN, PHASE_MERGE = 1, 2, 4
PHASE_ALL = 7
MAX_ENCODE_PROBES = 128  # nlsh_encode_hash generates up to this many keys per row; the scan takes them in slices of MAX_PROBES
EXACT_L2, EXACT_COSINE = 0, 1   # metrics of nlsh_exact_topk (precompute.py's forms: squared L2, 1 - cos; not the scan's METRIC_*)
PROBES = ("sampled", "ranked")  # multi-probe modes of the hashing: Philox Bernoulli draws (the reference's form, the default) | nlsh_probe_ranked
PROBE_RANKED_ROWS_PER_WORKGROUP = 4  # nlsh_probe_ranked: one wavefront per row, this many rows per workgroup (tests size their batches by it)
# NLSH_ENC_FORM_*: the kernel form nlsh_encode_hash takes for a shape (nlsh_encode_form reads the library's own choice back)
ENC_FORM_H16, ENC_FORM_SINGLE, ENC_FORM_SINGLE_WIDE, ENC_FORM_BUILD128, ENC_FORM_PINGPONG, ENC_FORM_HET = 0, 1, 2, 3, 4, 5
ENC_FORM_NAMES = ("H16", "SINGLE", "SINGLE_WIDE", "BUILD128", "PINGPONG", "HET")
MAX_BINS = 4096  # bins of a Categorical hash (NLSH_MAX_BINS): the widest output layer of nlsh_encode_logits, the widest row of nlsh_probe_bins
MAX_STREAM_WIDTH = 4096  # widest hidden layer of the streamed encoder form (nlsh_encode_hash_stream); MAX_WIDTH: the LDS-resident forms

# every symbol include/nlsh_hip.h declares (tests/test_host_cpu.py::test_capi_library_exports_every_declared_symbol checks the header against this)
SYMBOLS = (
    "nlsh_abi_version", "nlsh_last_error",
    "nlsh_encoder_packed_floats", "nlsh_encoder_pack", "nlsh_encode_hash", "nlsh_encode_form", "nlsh_pack_codes",
    "nlsh_encoder_stream_packed_floats", "nlsh_encoder_stream_pack", "nlsh_encode_stream_workspace", "nlsh_encode_hash_stream",
    "nlsh_build_csr_workspace", "nlsh_build_csr", "nlsh_bucket_order_workspace", "nlsh_bucket_order", "nlsh_build_cells_workspace", "nlsh_build_cells", "nlsh_gather_rows",
    "nlsh_scan_workspace", "nlsh_scan_workspace_layout", "nlsh_scan_topk", "nlsh_scan_topk_phase", "nlsh_scan_topk_cells_phase",
    "nlsh_merge_topk",
    "nlsh_step_create", "nlsh_step_create_graph", "nlsh_step_destroy", "nlsh_step_set_weights", "nlsh_query_step_enqueue", "nlsh_step_release", "nlsh_step_busy", "nlsh_query_batch",
    "nlsh_query_batch_host",
    "nlsh_exact_workspace", "nlsh_exact_topk",
    "nlsh_probe_ranked", "nlsh_probe_ranked_budget",
    "nlsh_logits_packed_floats", "nlsh_logits_pack", "nlsh_logits_workspace", "nlsh_encode_logits", "nlsh_probe_bins", "nlsh_probe_bins_budget",
    "nlsh_query_batch_ranked_scratch", "nlsh_query_batch_ranked",
    "nlsh_csr_update_workspace", "nlsh_csr_update",
    "nlsh_scan_topk_cells_phase_typed", "nlsh_gather_rows_typed", "nlsh_csr_update_typed",
    "nlsh_row_filter_words", "nlsh_row_filter_build", "nlsh_scan_topk_cells_phase_filtered",
    "nlsh_merge_topk_unique",
    "nlsh_range_workspace", "nlsh_range_sort_workspace", "nlsh_range_count", "nlsh_range_fill",
    "nlsh_sq8_train_workspace", "nlsh_sq8_train", "nlsh_gather_rows_sq8", "nlsh_csr_update_sq8", "nlsh_scan_topk_cells_phase_sq8",
    "nlsh_rerank_topk",
    "nlsh_scan_topk_cells_phase_tagged", "nlsh_scan_topk_cells_phase_sq8_tagged",
    "nlsh_pq_encode", "nlsh_pq_decode_rows", "nlsh_pq_inv_norm", "nlsh_scan_topk_cells_phase_pq",
)


class NlshHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"nlsh_hip error {code}: {msg}")
        self.code = code


_lib = None
vp, i32, i64, u64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t


class StepDesc(ctypes.Structure):
    """`nlsh_step_desc_t` of include/nlsh_hip.h, field for field (nlsh_step_create checks sizeof against the library's)."""
    _fields_ = [
        ("n_layers", ctypes.c_int32), ("act", ctypes.c_int32), ("key_mode", ctypes.c_int32), ("n_probes", ctypes.c_int32),
        ("dims", vp), ("packed", vp), ("n_multi_rows", i64),
        ("corpus_sorted", vp), ("row_stride", i64),
        ("gid", vp), ("uniq_keys", vp), ("offsets", vp), ("bucket_order", vp), ("cell_of", vp), ("cell_offsets", vp), ("inv_norm", vp),
        ("d", ctypes.c_int32), ("n_buckets", ctypes.c_int32), ("n_cells", ctypes.c_int32), ("k", ctypes.c_int32),
        ("metric", ctypes.c_int32), ("algo", ctypes.c_int32), ("seg_rows", ctypes.c_int32), ("hold_done", ctypes.c_int32),
        ("Q", i64), ("qkeys", vp), ("nkeys", vp), ("out_dist", vp), ("out_idx", vp), ("out_keys", vp), ("out_ncand", vp), ("status", vp),
        ("workspace", vp), ("workspace_bytes", sz), ("max_tasks", i64),
        ("front", vp), ("plan", vp), ("mid", vp), ("tail", vp),
    ]


def build_library(force=False):
    """Compile csrc/*.hip for gfx950 (hipcc cross-compiles without a GPU).  The optional list-construction helper is built for THIS
    interpreter (extension suffix and include directory from sysconfig), not for whichever python3-config is on PATH."""
    import sysconfig
    args = ["make", "-C", CSRC, "-j4"]
    suffix, inc = sysconfig.get_config_var("EXT_SUFFIX"), sysconfig.get_paths().get("include")
    if suffix and inc and os.path.exists(os.path.join(inc, "Python.h")):
        args += [f"PYSUFFIX={suffix}", f"PYINCLUDES=-I{inc}"]
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"])
    subprocess.check_call(args)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NlshHipError(E_HIP, f"{LIB_PATH} not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
                                  f"or `make -C {CSRC}`); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    L.nlsh_abi_version.restype = i32
    L.nlsh_last_error.restype = ctypes.c_char_p
    L.nlsh_encoder_packed_floats.restype = i64
    L.nlsh_encoder_packed_floats.argtypes = [i32, vp]
    L.nlsh_encoder_pack.restype = i32
    L.nlsh_encoder_pack.argtypes = [i32, vp, vp, vp, vp, vp]
    L.nlsh_encode_hash.restype = i32
    L.nlsh_encode_hash.argtypes = [vp, i64, i64, i32, vp, vp, i32, i32, i32, i64, u64, i64, vp, vp, vp, vp, vp, vp]
    L.nlsh_encode_form.restype = i32           # n, n_layers, dims, n_probes | form, rows per workgroup, LDS bytes, CUs (host pointers)
    L.nlsh_encode_form.argtypes = [i64, i32, vp, i32, vp, vp, vp, vp]
    L.nlsh_pack_codes.restype = i32
    L.nlsh_pack_codes.argtypes = [vp, i64, i32, i32, i32, vp, vp]
    L.nlsh_encoder_stream_packed_floats.restype = i64
    L.nlsh_encoder_stream_packed_floats.argtypes = [i32, vp]
    L.nlsh_encoder_stream_pack.restype = i32
    L.nlsh_encoder_stream_pack.argtypes = [i32, vp, vp, vp, vp, vp]
    L.nlsh_encode_stream_workspace.restype = sz
    L.nlsh_encode_stream_workspace.argtypes = [i64, i32, vp]
    L.nlsh_encode_hash_stream.restype = i32
    L.nlsh_encode_hash_stream.argtypes = list(L.nlsh_encode_hash.argtypes[:-1]) + [vp, sz, vp]
    L.nlsh_build_csr_workspace.restype = sz
    L.nlsh_build_csr_workspace.argtypes = [i64]
    L.nlsh_build_csr.restype = i32
    L.nlsh_build_csr.argtypes = [vp, i64, vp, vp, vp, vp, vp, sz, vp]
    L.nlsh_bucket_order_workspace.restype = sz
    L.nlsh_bucket_order_workspace.argtypes = [i64]
    L.nlsh_bucket_order.restype = i32
    L.nlsh_bucket_order.argtypes = [vp, i64, vp, vp, sz, vp]
    L.nlsh_build_cells_workspace.restype = sz
    L.nlsh_build_cells_workspace.argtypes = [i64]
    L.nlsh_build_cells.restype = i32
    L.nlsh_build_cells.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, sz, vp]
    L.nlsh_gather_rows.restype = i32
    L.nlsh_gather_rows.argtypes = [vp, i64, i32, vp, i64, vp, i64, vp, vp, ctypes.c_int32, vp]
    L.nlsh_csr_update_workspace.restype = sz
    L.nlsh_csr_update_workspace.argtypes = [i64, i64, i64]
    L.nlsh_csr_update.restype = i32     # old index (9) | keep, n_kept | new rows (5) | outputs (8) | workspace, bytes, stream
    L.nlsh_csr_update.argtypes = [vp, i64, i32, vp, vp, vp, vp, i64, i64,  vp, i64,  vp, i64, vp, vp, i64,
                                  vp, i64, vp, vp, vp, vp, vp, vp,  vp, sz, vp]
    L.nlsh_gather_rows_typed.restype = i32     # (corpus, storage) ... (sorted, storage) ... first_bad, stream
    L.nlsh_gather_rows_typed.argtypes = [vp, i32, i64, i32, vp, i64, vp, i32, i64, vp, vp, ctypes.c_int32, vp, vp]
    L.nlsh_csr_update_typed.restype = i32      # nlsh_csr_update with a storage behind corpus_sorted and rows_new, first_bad behind the outputs
    L.nlsh_csr_update_typed.argtypes = [vp, i32, i64, i32, vp, vp, vp, vp, i64, i64,  vp, i64,  vp, i32, i64, vp, vp, i64,
                                        vp, i64, vp, vp, vp, vp, vp, vp, vp,  vp, sz, vp]
    L.nlsh_scan_workspace.restype = sz
    L.nlsh_scan_workspace.argtypes = [i64, i32, i32, i64, i64, i32]
    L.nlsh_scan_workspace_layout.restype = i32
    L.nlsh_scan_workspace_layout.argtypes = [i64, i32, i32, i64, i64, i32, i32, vp, vp, vp]
    L.nlsh_scan_topk.restype = i32
    L.nlsh_scan_topk.argtypes = [vp, i64, i32, vp, vp, vp, vp, ctypes.c_int32, vp, vp, i64, i64, vp, vp, i32, i32, i32, i32, i32,
                                 vp, vp, vp, vp, vp, vp, sz, i64, vp, vp, vp]
    L.nlsh_scan_topk_phase.restype = i32
    L.nlsh_scan_topk_phase.argtypes = list(L.nlsh_scan_topk.argtypes) + [i32]
    L.nlsh_scan_topk_cells_phase.restype = i32     # cell_of, cell_offsets, n_cells follow n_buckets
    L.nlsh_scan_topk_cells_phase.argtypes = L.nlsh_scan_topk_phase.argtypes[:8] + [vp, vp, ctypes.c_int32] + L.nlsh_scan_topk_phase.argtypes[8:]
    L.nlsh_scan_topk_cells_phase_typed.restype = i32     # storage follows corpus_sorted
    L.nlsh_scan_topk_cells_phase_typed.argtypes = L.nlsh_scan_topk_cells_phase.argtypes[:1] + [i32] + L.nlsh_scan_topk_cells_phase.argtypes[1:]
    L.nlsh_scan_topk_cells_phase_filtered.restype = i32     # the typed call, row_filter behind phases
    L.nlsh_scan_topk_cells_phase_filtered.argtypes = L.nlsh_scan_topk_cells_phase_typed.argtypes + [vp]
    L.nlsh_range_workspace.restype = sz
    L.nlsh_range_workspace.argtypes = [i64, i32, i64, i64, i32]
    L.nlsh_range_sort_workspace.restype = sz
    L.nlsh_range_sort_workspace.argtypes = [i64, i64]
    # the filtered call's arguments up to nkeys, P | metric, algo | row_filter, radius | ...
    range_head = L.nlsh_scan_topk_cells_phase_filtered.argtypes[:19] + [i32, i32, vp, vp]
    L.nlsh_range_count.restype = i32     # ... out_count, out_ncand | status, workspace, bytes, max_tasks | scan events, stream
    L.nlsh_range_count.argtypes = range_head + [vp, vp, vp, vp, sz, i64, vp, vp, vp]
    L.nlsh_range_fill.restype = i32      # ... row_offsets, total, cursor | out_keys, out_dist, out_idx | status, workspace, bytes, max_tasks | sort workspace, bytes | scan events, stream
    L.nlsh_range_fill.argtypes = range_head + [vp, i64, vp, vp, vp, vp, vp, vp, sz, i64, vp, sz, vp, vp, vp]
    # storage="sq8": the uint8 layout plus (lo, step); entry points of their own, the typed calls keep refusing storage codes past STORE_U8
    L.nlsh_sq8_train_workspace.restype = sz
    L.nlsh_sq8_train_workspace.argtypes = [i64, i32]
    L.nlsh_sq8_train.restype = i32             # rows, storage, row_stride, d, n | lo, step, quant_stride | first_bad | workspace, bytes, stream
    L.nlsh_sq8_train.argtypes = [vp, i32, i64, i32, i64, vp, vp, i64, vp, vp, sz, vp]
    L.nlsh_gather_rows_sq8.restype = i32       # (corpus, storage) ... sorted, dst_stride, lo, step ... first_bad, clamped_rows, stream
    L.nlsh_gather_rows_sq8.argtypes = [vp, i32, i64, i32, vp, i64, vp, i64, vp, vp, vp, vp, ctypes.c_int32, vp, vp, vp]
    L.nlsh_csr_update_sq8.restype = i32        # the typed update with (lo, step) in place of the storage code and clamped_rows behind first_bad
    L.nlsh_csr_update_sq8.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp, vp, i64, i64,  vp, i64,  vp, i32, i64, vp, vp, i64,
                                      vp, i64, vp, vp, vp, vp, vp, vp, vp, vp,  vp, sz, vp]
    L.nlsh_scan_topk_cells_phase_sq8.restype = i32     # the filtered call with (lo, step) in place of the storage code
    L.nlsh_scan_topk_cells_phase_sq8.argtypes = (L.nlsh_scan_topk_cells_phase_filtered.argtypes[:1] + [vp, vp]
                                                 + L.nlsh_scan_topk_cells_phase_filtered.argtypes[2:])
    for base in ("nlsh_scan_topk_cells_phase_filtered", "nlsh_scan_topk_cells_phase_sq8"):     # ... plus row_tags, query_masks, tag_match
        tagged = getattr(L, base.replace("_filtered", "") + "_tagged")
        tagged.restype = i32
        tagged.argtypes = list(getattr(L, base).argtypes) + [vp, vp, i32]
    # storage="pq": code rows plus a codebook; the sorted copy moves through the typed uint8 calls, the scan has an entry of its own
    L.nlsh_pq_encode.restype = i32             # rows, storage, row_stride, d, n | codebook, dsub | codes, code_pitch | first_bad, stream
    L.nlsh_pq_encode.argtypes = [vp, i32, i64, i32, i64, vp, i32, vp, i64, vp, vp]
    L.nlsh_pq_decode_rows.restype = i32        # codes, code_pitch, n | codebook, dsub, d | out, out_stride, stream
    L.nlsh_pq_decode_rows.argtypes = [vp, i64, i64, vp, i32, i32, vp, i64, vp]
    L.nlsh_pq_inv_norm.restype = i32           # codes, code_pitch, n | codebook, dsub, d | inv_norm, stream
    L.nlsh_pq_inv_norm.argtypes = [vp, i64, i64, vp, i32, i32, vp, vp]
    L.nlsh_scan_topk_cells_phase_pq.restype = i32      # the filtered call with (codebook, dsub, code_pitch) in place of the storage code
    L.nlsh_scan_topk_cells_phase_pq.argtypes = (L.nlsh_scan_topk_cells_phase_filtered.argtypes[:1] + [vp, i32, i64]
                                                + L.nlsh_scan_topk_cells_phase_filtered.argtypes[2:])
    L.nlsh_row_filter_words.restype = sz
    L.nlsh_row_filter_words.argtypes = [i64]
    L.nlsh_row_filter_build.restype = i32      # gid, n_rows | ids, n_ids | dense, n_dense, id_base | invert | row_filter, n_allowed, stream
    L.nlsh_row_filter_build.argtypes = [vp, i64, vp, i64, vp, i64, ctypes.c_int32, i32, vp, vp, vp]
    L.nlsh_merge_topk.restype = i32
    L.nlsh_merge_topk.argtypes = [vp, i64, i32, i64, i32, vp, vp, vp, vp, vp]
    L.nlsh_merge_topk_unique.restype = i32     # nlsh_merge_topk with out_keys in front of out_ncand
    L.nlsh_merge_topk_unique.argtypes = [vp, i64, i32, i64, i32, vp, vp, vp, vp, vp, vp]
    L.nlsh_rerank_topk.restype = i32           # queries (4) | store (5), inv_norm | cand, stride, kc, k, metric | outputs (4), first_bad, stream
    L.nlsh_rerank_topk.argtypes = [vp, i64, i64, i32,  vp, i64, i64, ctypes.c_int32, i32, vp,  vp, i64, i32, i32, i32,  vp, vp, vp, vp, vp, vp]
    L.nlsh_step_create.restype = i32
    L.nlsh_step_create.argtypes = [ctypes.POINTER(StepDesc), sz, ctypes.POINTER(vp)]
    L.nlsh_step_create_graph.restype = i32
    L.nlsh_step_create_graph.argtypes = [ctypes.POINTER(StepDesc), sz, vp, ctypes.POINTER(vp)]
    for name in ("nlsh_step_destroy", "nlsh_step_release", "nlsh_step_busy"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [vp]
    L.nlsh_step_set_weights.restype = i32
    L.nlsh_step_set_weights.argtypes = [vp, vp]
    L.nlsh_query_step_enqueue.restype = i32
    L.nlsh_query_step_enqueue.argtypes = [vp, vp, i64, u64, vp, vp, vp]
    L.nlsh_query_batch.restype = i32
    L.nlsh_query_batch.argtypes = [ctypes.POINTER(StepDesc), sz, vp, i64, u64, i64, i32, vp, vp, vp]
    L.nlsh_query_batch_host.restype = i32
    L.nlsh_query_batch_host.argtypes = [ctypes.POINTER(StepDesc), sz, vp, i64, u64, i64, i32, vp, sz, vp]
    L.nlsh_exact_workspace.restype = sz
    L.nlsh_exact_workspace.argtypes = [i64, i64, i32, i32]
    L.nlsh_exact_topk.restype = i32
    L.nlsh_exact_topk.argtypes = [vp, i64, i64, i32, vp, i64, i64, i32, i32, i64, i32, vp, vp, vp, sz, vp]
    L.nlsh_probe_ranked.restype = i32
    L.nlsh_probe_ranked.argtypes = [vp, i64, vp, i64, i32, i32, i32, i64, vp, vp, vp, vp]
    L.nlsh_probe_ranked_budget.restype = i32
    L.nlsh_probe_ranked_budget.argtypes = [vp, i64, vp, i64, i32, i32, i32, i64, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.nlsh_logits_packed_floats.restype = i64
    L.nlsh_logits_packed_floats.argtypes = [i32, vp]
    L.nlsh_logits_pack.restype = i32
    L.nlsh_logits_pack.argtypes = [i32, vp, vp, vp, vp, vp]
    L.nlsh_logits_workspace.restype = sz
    L.nlsh_logits_workspace.argtypes = [i64, i32, vp]
    L.nlsh_encode_logits.restype = i32          # x, n, x_stride | n_layers, dims, packed | logits_out, logits_stride | workspace, bytes, stream
    L.nlsh_encode_logits.argtypes = [vp, i64, i64, i32, vp, vp, vp, i64, vp, sz, vp]
    L.nlsh_probe_bins.restype = i32             # logits, stride, n, M, n_probes, n_multi_rows | keys_out, nkeys_out, logit_out, stream
    L.nlsh_probe_bins.argtypes = [vp, i64, i64, i32, i32, i64, vp, vp, vp, vp]
    L.nlsh_probe_bins_budget.restype = i32      # ... n_multi_rows | uniq_keys, offsets, n_buckets, budget | keys_out, nkeys_out, logit_out, ncand_out, stream
    L.nlsh_probe_bins_budget.argtypes = [vp, i64, i64, i32, i32, i64, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.nlsh_query_batch_ranked_scratch.restype = sz
    L.nlsh_query_batch_ranked_scratch.argtypes = [i64, i32]
    L.nlsh_query_batch_ranked.restype = i32     # desc, sizeof(desc), queries, q_stride, lookup_done, budget, scratch, bytes, host_out, words, scan events, stream
    L.nlsh_query_batch_ranked.argtypes = [ctypes.POINTER(StepDesc), sz, vp, i64, i32, ctypes.c_int32, vp, sz, vp, sz, vp, vp, vp]
    _lib = L
    return L


def check(rc):
    if rc != OK:
        raise NlshHipError(rc, lib().nlsh_last_error().decode("utf-8", "replace"))


def encode_form(n, dims, n_probes=1):
    """(form id, rows per workgroup, LDS bytes per workgroup, CU count of the HET rule) of the `nlsh_encode_hash` call of `n` rows
    through the layer stack `dims` = [d, hidden..., H]: the library's own plan, nothing is launched.  A refused shape raises."""
    form, rows, cus, lds = i32(-1), i32(0), i32(0), sz(0)
    check(lib().nlsh_encode_form(int(n), len(dims) - 1, int_array(dims), int(n_probes), ctypes.byref(form), ctypes.byref(rows),
                                 ctypes.byref(lds), ctypes.byref(cus)))
    return form.value, rows.value, lds.value, cus.value


def probe_mode(probes, default="sampled"):
    """The multi-probe mode of a call: `probes` when given, else `default`; anything but "sampled" / "ranked" is a ValueError."""
    mode = default if probes is None else probes
    if mode not in PROBES:
        raise ValueError(f"probes must be one of {PROBES}, got {mode!r}")
    return mode


def ptr(t):
    """Device (or host) pointer of a torch tensor / None."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def int_array(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])
