"""`build_index` / `Indexer` with the reference's surface (nlsh/indexer.py:6-96) on gfx950.

Index build: hash the corpus on the device (`encode_hash`), stable radix sort of (key, row)
-> CSR (`perm`, `uniq_keys`, `offsets`) and a bucket-contiguous copy of the corpus.
Query: ONE `encode_hash` launch for the whole batch (multi-probe keys stay on the device) and
ONE `nlsh_scan_topk` call (plan -> scan -> merge kernels) instead of the reference's per-query
Python loop with ~(P+4) launches and a device sync per query.

`query()` returns the reference's `(List[List[int]], List[int])`; `query_tensors()` is the same
computation with device-resident results (what bench.py times).  compat=True (default) keeps the
reference quirks: int16 key wrap (F2), single-probe trailing partial batch (F6), `<k` fallback =
last key's bucket rows (F7).  No CPU fallback exists anywhere in this module.
"""
import contextlib
import ctypes
import gc
import numbers
import operator
import threading
import weakref
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np
import torch

from . import _capi
from .data import metric_of
from .refine import RefineStore, checked_refine, stage_one_k
from .hashings import host_key_set, keys_to_sets

HASH_BATCH = 4096  # nlsh/indexer.py:40 default batch_size


class _CollectorPause:
    """The cyclic collector paused for a region, re-entrant and shared by every thread of the process (the collector's switch is one
    process-wide flag, so the pause has to be one process-wide object): the FIRST region to open records the state the application
    left the collector in and disables it, regions opened meanwhile -- nested in the same thread (`query` -> `_plain_lists`) or by
    `query()` calls of other threads -- only count, and the LAST one to close restores what the first one found.  A caller that had
    the collector disabled gets it back disabled; a caller that enables it while a region is open keeps it enabled (the exit only
    ever ENABLES, and only when the pause itself disabled).  What the gc module cannot show is another thread calling
    `gc.disable()` while a region is open (a no-op on an already disabled collector): that thread finds the collector enabled again
    once the last region closes -- INTEGRATION.md says so.

    `application_state()` is the collector state the application chose: what the first open region found, `gc.isenabled()` when none
    is open.  `Indexer.promote_results` asks it (inside a paused `query()` `gc.isenabled()` is always False)."""

    def __init__(self):
        self._lock = threading.Lock()
        self._depth = 0
        self._found_enabled = False

    def __enter__(self):
        with self._lock:
            if self._depth == 0:
                self._found_enabled = gc.isenabled()
                if self._found_enabled:
                    gc.disable()
            self._depth += 1
        return self

    def __exit__(self, *exc):
        with self._lock:
            self._depth -= 1
            if self._depth == 0 and self._found_enabled:
                self._found_enabled = False
                gc.enable()
        return False

    def application_state(self):
        with self._lock:
            return self._found_enabled if self._depth else gc.isenabled()


_collector_pause = _CollectorPause()


def _load_fastlists():
    """csrc/fastlists.c (built by the Makefile next to the HIP library): the result lists in one tight C loop.  Host-side and
    optional -- `ndarray.tolist()` builds the identical lists -- unlike the HIP library, which has no substitute."""
    import importlib.machinery
    import importlib.util
    import os
    # only a build for THIS interpreter's ABI (the Makefile names the file with `python3-config --extension-suffix`)
    path = os.path.join(os.path.dirname(_capi.LIB_PATH), "_nlsh_fastlists" + importlib.machinery.EXTENSION_SUFFIXES[0])
    if not os.path.exists(path):
        return None
    try:
        spec = importlib.util.spec_from_file_location("_nlsh_fastlists", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    except (ImportError, OSError):
        return None


_fastlists = _load_fastlists()
_rows_to_lists = getattr(_fastlists, "rows_to_lists", None)
# the two-phase construction of `query()`'s lists (csrc/fastlists.c: the containers while the device scans, the ids per row range);
# None (helper not built, or built from an older source) = the one-shot conversion, `_plain_lists`
_rows_alloc, _rows_fill = getattr(_fastlists, "rows_alloc", None), getattr(_fastlists, "rows_fill", None)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _addr(t):
    """Address of a tensor that may be absent."""
    return None if t is None else t.data_ptr()


def _event_handles(events):
    """The (begin, end) handles of a call's `events=` pair, (None, None) without one."""
    return (events[0].cuda_event, events[1].cuda_event) if events else (None, None)


_no_pause = contextlib.nullcontext()    # `query()` with `pause_collector_for_call` off: one object for every call, it holds no state


# `nlsh_scan_topk_cells_phase`'s arguments either side of (queries, q_stride), by their names in `Indexer._scan_fields`
_SCAN_ARGS_BEFORE_QUERIES = operator.itemgetter("corpus_sorted", "row_stride", "d", "gid", "uniq_keys", "offsets", "bucket_order", "n_buckets",
                                                "cell_of", "cell_offsets", "n_cells", "inv_norm")
_SCAN_ARGS_AFTER_QUERIES = operator.itemgetter("Q", "qkeys", "nkeys", "n_probes", "k", "metric", "algo", "seg_rows", "out_dist", "out_idx", "out_keys",
                                               "out_ncand", "status", "workspace", "workspace_bytes", "max_tasks")


def build_csr_device(keys: torch.Tensor):
    """int32 keys [N] (device) -> (perm int32 [N], uniq_keys int32 [nb], offsets int32 [nb+1])."""
    L = _capi.lib()
    keys = keys.contiguous()
    n = keys.shape[0]
    dev = keys.device
    perm = torch.empty((n,), dtype=torch.int32, device=dev)
    uniq = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    offs = torch.empty((n + 1,), dtype=torch.int32, device=dev)
    nb = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws_bytes = L.nlsh_build_csr_workspace(n)
    if ws_bytes == 0:
        _capi.check(_capi.E_HIP)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    _capi.check(L.nlsh_build_csr(_capi.ptr(keys), n, _capi.ptr(perm), _capi.ptr(uniq), _capi.ptr(offs), _capi.ptr(nb),
                                 _capi.ptr(ws), ws_bytes, _stream(dev)))
    n_buckets = int(nb.item())  # index build may synchronise; the query path never does
    return perm, uniq[:n_buckets], offs[:n_buckets + 1]


def build_index(indexes, cuda=True) -> Dict[int, torch.Tensor]:
    """nlsh/indexer.py:6-24: {key: LongTensor of the rows whose key set contains it, ascending}.

    cuda=True sorts the (key, row) pairs with the device radix sort; cuda=False is the host-only
    variant the reference's own unit test uses (nlsh/tests/test_indexer.py) and needs no GPU.
    """
    rows, keys = [], []
    for row, key_set in enumerate(indexes):
        for key in key_set:
            rows.append(row)
            keys.append(int(key))
    if not keys:
        return {}
    keys_np = np.asarray(keys, dtype=np.int64)
    rows_t = torch.as_tensor(np.asarray(rows, dtype=np.int64))
    if cuda:
        if keys_np.min() < -(1 << 31) or keys_np.max() >= (1 << 32):
            raise ValueError("bucket keys must fit 32 bits")
        k32 = torch.as_tensor(keys_np.astype(np.uint32).view(np.int32) if keys_np.max() >= (1 << 31)
                              else keys_np.astype(np.int32)).cuda()
        perm, uniq, offs = build_csr_device(k32)
        grouped = rows_t.cuda()[perm.long()]
        sizes = torch.diff(offs).cpu().tolist()
        # report keys as the caller passed them (first pair of each bucket)
        first = perm[offs[:-1].long()].cpu().numpy()
        names = keys_np[first].tolist()
    else:
        order = torch.sort(torch.as_tensor(keys_np), stable=True)
        uniq, counts = torch.unique_consecutive(order.values, return_counts=True)
        grouped = rows_t[order.indices]
        sizes = counts.tolist()
        names = uniq.tolist()
    return {int(k): chunk for k, chunk in zip(names, torch.split(grouped, sizes))}


# `storage=`: element type of the bucket-sorted corpus copy -> (torch dtype, NLSH_STORE_* code, elements per 16 bytes)
#   "sq8" holds uint8 CODES in the uint8 layout and decodes them with the index's per-dimension quantiser: its calls
#   are the *_sq8 entry points, the typed ones never see it
_STORAGES = {"float32": (torch.float32, _capi.STORE_F32, 4), "float16": (torch.float16, _capi.STORE_F16, 8), "uint8": (torch.uint8, _capi.STORE_U8, 16),
             "sq8": (torch.uint8, _capi.STORE_U8, 16), "pq": (torch.uint8, _capi.STORE_U8, 16)}
#   "pq" holds product-quantiser CODES, M = ceil(d / dsub) bytes per row, decoded through the index's codebook: the
#   sorted copy moves through the typed uint8 calls at width M, the scan has the *_pq entry point
PQ_DSUBS = (4, 8, 16)
_STORE_CODE_OF_DTYPE = {dt: code for dt, code, _ in _STORAGES.values()}


def checked_codebook(codebook, d, dsub):
    """`quantiser=` of a pq index, checked on the host before anything touches a device -> the codebook, float32 [M, 256, dsub]
    contiguous (on whatever device it came from), the columns of the last sub-vector at or beyond d zeroed (a copy if any had to be)."""
    M = (d + dsub - 1) // dsub
    if isinstance(codebook, (tuple, list)):
        raise ValueError(f"quantiser of storage='pq' must be a codebook, a float32 [{M}, 256, {dsub}] array, not a {type(codebook).__name__}")
    t = codebook if isinstance(codebook, torch.Tensor) else torch.as_tensor(np.asarray(codebook))
    if t.dtype != torch.float32:
        raise ValueError(f"codebook must be float32, got {t.dtype}")
    if tuple(t.shape) != (M, 256, dsub):
        raise ValueError(f"codebook must have shape ({M}, 256, {dsub}) for d={d}, pq_dsub={dsub}, got {tuple(t.shape)}")
    if t.device.type == "cpu" and not bool(torch.isfinite(t).all()):       # (a device codebook is held against this where the index is built)
        raise ValueError("codebook must be finite")
    tail = M * dsub - d
    t = t.contiguous()
    if tail and bool((t[M - 1, :, dsub - tail:] != 0).any() if t.device.type == "cpu" else True):
        t = t.clone()
        t[M - 1, :, dsub - tail:] = 0.0
    return t


def checked_quantiser(quantiser, d):
    """`quantiser=` of an sq8 index, checked on the host before anything touches a device -> (lo, step) float32 [d] host tensors."""
    if not isinstance(quantiser, (tuple, list)) or len(quantiser) != 2:
        raise ValueError("quantiser must be a pair (lo, step) of float32 [d] arrays")
    out = []
    for name, v in zip(("lo", "step"), quantiser):
        t = torch.as_tensor(v)
        if t.dtype != torch.float32:
            raise ValueError(f"quantiser {name} must be float32, got {t.dtype}")
        if tuple(t.shape) != (d,):
            raise ValueError(f"quantiser {name} must have shape ({d},), got {tuple(t.shape)}")
        t = t.detach().cpu().contiguous()
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"quantiser {name} must be finite")
        out.append(t)
    if not bool((out[1] > 0).all()):
        raise ValueError("quantiser step must be > 0 in every dimension")
    return out[0], out[1]


class RowFilter:
    """A row allow/deny filter of ONE index in ONE generation (`Indexer.row_filter` builds it): `words`, the device
    bitset over the index's bucket-sorted rows (int32 tensor holding the uint32 words of include/nlsh_hip.h: bit p & 31 of word p >> 5
    = sorted row p may be returned), `n_allowed`, how many rows it allows, and `generation`, the index's when it was built.  Reusable
    across calls (`filter=`); stale after an effective `add` / `remove` / `update`, which move rows: build a new one."""

    __slots__ = ("words", "n_allowed", "generation", "_index")

    def __init__(self, index, words, n_allowed, generation):
        self.words, self.n_allowed, self.generation = words, int(n_allowed), int(generation)
        self._index = weakref.ref(index)

    def __repr__(self):
        return f"RowFilter(n_allowed={self.n_allowed}, generation={self.generation})"


TAG_MATCH = {"any": _capi.TAG_ANY, "all": _capi.TAG_ALL, "eq": _capi.TAG_EQ}   # tag_match= -> NLSH_TAG_* (include/nlsh_hip.h)


class TagFilter:
    """What a tagged call carries where an untagged one carries its `RowFilter` (internal; built by `Indexer._checked_filter` from
    `tag_mask=` / `tag_match=` / `filter=`): `mask`, one Python int for every query or an int64 [Q] device tensor, `match`, the
    NLSH_TAG_* code, and `row_filter`, the checked RowFilter or None (a row must pass both).  DESIGN.md 4.16."""

    __slots__ = ("mask", "match", "row_filter")

    def __init__(self, mask, match, row_filter):
        self.mask, self.match, self.row_filter = mask, int(match), row_filter

    def masks(self, Q, dev):
        """int64 [Q] on `dev`: the tensor as given, or the one int repeated."""
        if isinstance(self.mask, torch.Tensor):
            return self.mask
        return torch.full((max(Q, 1),), self.mask, dtype=torch.int64, device=dev)


def checked_tags(tags, n_rows, dev, what="tags"):
    """A tag array of the constructor / `add` / `set_tags`: int64 [n_rows] on the index's device (the 64 bits are read as unsigned)."""
    if not isinstance(tags, torch.Tensor) or tags.dtype != torch.int64 or tuple(tags.shape) != (n_rows,):
        got = f"{tags.dtype} {tuple(tags.shape)}" if isinstance(tags, torch.Tensor) else type(tags).__name__
        raise ValueError(f"{what} must be an int64 tensor of shape ({n_rows},) (64 tag bits per row, read as unsigned), got {got}")
    if tags.device != dev:
        raise ValueError(f"{what} are on {tags.device}, the index on {dev}")
    return tags.contiguous()


def pack_row_filter(allowed) -> np.ndarray:
    """Host statement of the filter layout: bool [N] in sorted-row order -> uint32 [2 * ceil(N / 64)] words (what
    `nlsh_row_filter_build` writes on the device; the tests hold one against the other)."""
    allowed = np.asarray(allowed, dtype=bool).reshape(-1)
    n_words = 2 * ((allowed.shape[0] + 63) // 64)
    bits = np.zeros((n_words * 32,), dtype=np.uint8)
    bits[:allowed.shape[0]] = allowed
    return np.packbits(bits.reshape(n_words, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


def pq_encode(rows, codebook, d, what="rows", row_base=0):
    """Float rows [n, d] (device; float32 or float16, anything else is converted with `.float()`) -> their product-quantiser codes, uint8
    [n, M], by `nlsh_pq_encode` -- the one statement of the encoding rule on the device (include/nlsh_hip.h).  `codebook`: float32
    [M, 256, dsub] on the rows' device.  A row holding a NaN or an infinity raises ValueError naming `what` row `row_base` + its number."""
    if rows.dtype not in (torch.float32, torch.float16):
        rows = rows.float()
    if rows.dim() != 2 or rows.stride(1) != 1:
        rows = rows.contiguous()
    n, dev, M, dsub = int(rows.shape[0]), rows.device, int(codebook.shape[0]), int(codebook.shape[2])
    codes = torch.empty((n, M), dtype=torch.uint8, device=dev)
    first_bad = torch.empty((1,), dtype=torch.int32, device=dev)
    _capi.check(_capi.lib().nlsh_pq_encode(_capi.ptr(rows), _STORE_CODE_OF_DTYPE[rows.dtype], rows.stride(0) if n else d, d, n, _capi.ptr(codebook),
                                           dsub, _capi.ptr(codes), M, _capi.ptr(first_bad), _stream(dev)))
    bad = int(first_bad.item())
    if bad >= 0:
        Indexer._raise_unrepresentable(row_base + bad, "pq", what)
    return codes


def pq_decode(codes, codebook, d):
    """Codes uint8 [n, >= M] (device, unit column stride, any pitch) -> the decoded rows, float32 [n, d], by `nlsh_pq_decode_rows`: element j
    of a row is codebook[j // dsub][code[j // dsub]][j % dsub], a copy."""
    if codes.stride(1) != 1:
        codes = codes.contiguous()
    n, dev, dsub = int(codes.shape[0]), codes.device, int(codebook.shape[2])
    out = torch.empty((n, d), dtype=torch.float32, device=dev)
    _capi.check(_capi.lib().nlsh_pq_decode_rows(_capi.ptr(codes), codes.stride(0) if n else int(codebook.shape[0]), n, _capi.ptr(codebook), dsub, d,
                                                _capi.ptr(out), d, _stream(dev)))
    return out


class Indexer:

    # "float32" | "float16" | "uint8": what `corpus_sorted` holds.  A compressed index (the last two) is, by definition,
    # the float32 index over its dequantised rows: both conversions to float32 are exact, the rows are widened as the tiled scan stages
    # them, and every array and every query result has the float32 index's bits.
    storage = "float32"
    # None | "device" | "host": where the index keeps the caller's float32 rows for the exact re-rank; None = no second stage
    refine, refine_factor, refine_store = None, 4, None
    # None | int64 [N]: the rows' 64-bit tag words in SORTED order, beside `gid` (an index built with `tags=`)
    tags_sorted = None

    def __init__(self, hashing, candidate_vectors_gpu, distance_func, compat=True, metric: Optional[str] = None,
                 seg_rows: int = 0, id_base: int = 0, algo: Optional[str] = None,
                 row_ids: Optional[torch.Tensor] = None, schedule_stats: Optional[Tuple[float, float]] = None,
                 corpus_keys: Optional[torch.Tensor] = None, l2_form: str = "exact", window_rows: Optional[int] = None,
                 row_align: int = 4, storage: Optional[str] = None, quantiser=None, refine: Optional[str] = None, refine_factor: int = 4,
                 tags: Optional[torch.Tensor] = None, pq_dsub: Optional[int] = None, pq_dim: Optional[int] = None):
        # tags: None | int64 [N] in the caller's row order = one 64-bit tag word per row for per-query tag filters (`tag_mask=` of the
        # query calls).  The index keeps them beside `gid` in sorted order (`tags_sorted`, 8 bytes per row) and carries
        # them through add / remove / update; an index built without tags has none and refuses `tag_mask=` and `add(tags=)`.
        self._given_tags = None if tags is None else checked_tags(tags, int(candidate_vectors_gpu.shape[0]), candidate_vectors_gpu.device)
        self.tags_sorted = None
        # refine: None | "device" | "host" = keep the caller's rows as float32 in id order (`RefineStore`) and rescore every
        # top-k call's candidates on them: stage one runs at k1 = min(256, max(k, refine_factor * k)), one `nlsh_rerank_topk` launch cuts
        # to k.  The store addresses rows by id - id_base: custom ids (`row_ids=`, `add(ids=)`) are refused, here and there.
        self.refine, self.refine_factor = checked_refine(refine, refine_factor)
        self.refine_store = None
        if self.refine is not None and row_ids is not None:
            raise ValueError("refine= needs the default row ids (id_base + row): the refine store addresses a row by id - id_base, "
                             "row_ids= names rows freely")
        # storage: None / "float32" = the float32 copy (any other corpus dtype is converted with `.float()`, as ever); "float16" /
        # "uint8" / "sq8" = a compressed copy, read by the tiled schedule only (checked before anything touches a device)
        if storage is not None and storage not in _STORAGES:
            raise ValueError(f"storage must be None or one of {tuple(_STORAGES)}, got {storage!r}")
        self.storage = storage or "float32"
        if self.compressed and algo in ("query", "bucket"):
            raise ValueError(f"algo={algo!r} cannot read storage={self.storage!r}: a compressed index is scanned by the tiled schedule only "
                             "(algo=None or 'tiled')")
        # quantiser (storage="sq8" only): None = train on the (float) corpus; (lo, step), float32 [d] = use it.  A uint8 corpus is codes
        # and has nothing to train on.
        if quantiser is not None and self.storage not in ("sq8", "pq"):
            raise ValueError(f"quantiser= belongs to storage='sq8' (lo, step) or storage='pq' (a codebook), not storage={self.storage!r}")
        self._quantiser_given = None
        # storage="pq" (DESIGN.md 4.18): pq_dsub = width of a sub-vector (4 | 8 | 16, default 8); quantiser = None (train a codebook on
        # the float corpus) or the codebook, float32 [M, 256, pq_dsub].  A uint8 [N, M] corpus IS codes and needs the codebook; its row
        # width is then M * pq_dsub unless pq_dim names a d with a partial last sub-vector.
        if (pq_dsub is not None or pq_dim is not None) and self.storage != "pq":
            raise ValueError(f"pq_dsub= / pq_dim= belong to storage='pq', not storage={self.storage!r}")
        self.pq_dsub = None
        if self.storage == "pq":
            self.pq_dsub = 8 if pq_dsub is None else pq_dsub
            if isinstance(self.pq_dsub, bool) or self.pq_dsub not in PQ_DSUBS:
                raise ValueError(f"pq_dsub must be one of {PQ_DSUBS}, got {pq_dsub!r}")
            if tags is not None:
                raise NotImplementedError("tags= is not built for storage='pq': the tagged kernels read no codebook (DESIGN.md 7)")
            is_codes = candidate_vectors_gpu.dtype == torch.uint8
            if is_codes and quantiser is None:
                raise ValueError("a uint8 corpus is pq codes: storage='pq' needs quantiser=codebook to decode them")
            width = int(candidate_vectors_gpu.shape[1])
            d_pq = (width * self.pq_dsub if is_codes else width) if pq_dim is None else int(pq_dim)
            if is_codes and (d_pq + self.pq_dsub - 1) // self.pq_dsub != width:
                raise ValueError(f"pq_dim={d_pq} at pq_dsub={self.pq_dsub} is {(d_pq + self.pq_dsub - 1) // self.pq_dsub} code bytes per row, the corpus has {width}")
            if not is_codes and d_pq != width:
                raise ValueError(f"pq_dim={d_pq} != the corpus width {width}")
            self._pq_dim = d_pq
            if quantiser is not None:
                self._quantiser_given = checked_codebook(quantiser, d_pq, self.pq_dsub)
        if self.storage == "sq8":
            if quantiser is not None:
                self._quantiser_given = checked_quantiser(quantiser, int(candidate_vectors_gpu.shape[1]))
            elif candidate_vectors_gpu.dtype == torch.uint8:
                raise ValueError("a uint8 corpus is sq8 codes: storage='sq8' needs quantiser=(lo, step) to decode them")
        self.last_clamped_rows = 0  # sq8: rows of the last encode (build / add / update) with at least one saturated element
        self._hashing = hashing
        self._candidate_vectors_gpu = candidate_vectors_gpu
        self._distance_func = distance_func
        self.compat = compat
        self.metric = metric or metric_of(distance_func)
        self.seg_rows = seg_rows
        self.algo = algo            # None = choose per batch; "query" | "bucket" | "tiled" force a schedule
        # (size-biased bucket size, row count) of the WHOLE corpus when this index holds a shard of it (the sharded
        # builds compute them from the all-gathered keys): the schedule is chosen from whole-corpus statistics, so every
        # shard count runs the same arithmetic and results stay bit-identical
        self.schedule_stats = schedule_stats
        self.id_base = int(id_base)
        # global row id of every local row (int32 [N], device) when the shard is not a contiguous range
        # (bucket-sharded corpus); default: id_base + local row
        self.row_ids = row_ids
        # bucket key of every row (int32 [N], device) when the caller already has them (keys recorded by another run of
        # the same hash: parity on an identical index); default: hash the corpus here (indexer.py:36-38)
        self._given_keys = corpus_keys
        # "exact" (default): sqrt(sum(((q - c) + 1e-6)^2)) in F.pairwise_distance's operation order, bit-identical to the oracle.
        # "folded" (opt-in, NLSH_METRIC_L2_EPS_FOLDED): sqrt(sum(((q + 1e-6) - c)^2)) -- 2 instead of 3 vector operations per element in
        # the LDS-tiled schedule, one rounding per element away from the reference's order (|d - d_exact| <= 1e-4 * max(1, d))
        if l2_form not in ("exact", "folded"):
            raise ValueError("l2_form must be 'exact' or 'folded'")
        self.l2_form = l2_form
        # Small-bucket packing of the tiled schedule (include/nlsh_hip.h, nlsh_build_cells): consecutive buckets of <= window_rows rows
        # share one row window and its tasks.  None = choose per batch (`choose_window`), 0 = off (one task list per bucket, r03),
        # 64 / 128 / 256 = forced.  Never changes a result bit, only the number of tasks.
        if window_rows is not None and not 0 <= int(window_rows) <= 256:
            raise ValueError("window_rows must be None (auto) or in [0, 256]")
        self.window_rows = None if window_rows is None else int(window_rows)
        # Row stride of the bucket-sorted corpus copy, in floats: ceil(d / row_align) * row_align.  4 (default) packs rows at 16-byte
        # granularity; 32 starts every row on a 128-byte line of the L2 at the price of padding (100-d: 400 -> 512 bytes per row).
        # Never changes a result (padding columns are never read: the kernels walk d, not the stride).
        if row_align % 4 or row_align < 4:
            raise ValueError("row_align must be a multiple of 4 floats")
        self.row_align = int(row_align)
        self._cells = {}            # window_rows -> (cell_of, cell_offsets, cell_order, n_cells), built on first use
        self._index2row = None
        self._perm_host = None
        self._e_sb = None
        self._pin = None            # pinned host staging of query()'s single device->host copy
        self._ws = {}               # scan workspace per stream (concurrent query batches on different HIP streams)
        self._max_tasks = {}
        self.generation = 0         # +1 per effective `update` / `add` / `remove`: what was built on the arrays of an older one is stale
        self._build_index()
        # the id `add` gives its first row when the caller names none: only ever grows, so a removed row's id is never handed out again
        self.next_id = self.id_base + int(self.gid.shape[0])
        if self.refine is not None:
            if self.metric not in ("l2", "cosine"):
                raise NotImplementedError("refine= needs metric 'l2' or 'cosine': the re-rank kernel computes the distance")
            # the caller's rows BEFORE they are compressed (sq8 codes have no other original than what they decode to)
            originals = candidate_vectors_gpu
            if self.storage in ("sq8", "pq") and originals.dtype == torch.uint8:
                originals = self._dequantised(originals)
            self.refine_store = RefineStore(originals, self.metric, id_base=self.id_base, where=self.refine, row_align=self.row_align)

    @property
    def compressed(self):
        return self.storage != "float32"

    def _dequantised(self, rows, row_base=0):
        """Rows as the index holds them, in float32: `rows.to(storage).float()` (both steps exact on representable values)."""
        if self.storage == "pq":
            # codes decode as they are; anything else is encoded first (`nlsh_pq_encode`), then `nlsh_pq_decode_rows`: a copy out of the codebook
            codes = rows if rows.dtype == torch.uint8 else self._pq_encode(rows, "corpus", row_base)
            return self._pq_decode(codes)
        if self.storage == "sq8":
            # codes decode as they are; anything else is encoded first (the library's kernel: the one statement of the rule on the
            # device) -- deq(c, j) = float(c) * step[j] + lo[j] as two separately rounded torch operations
            codes = rows if rows.dtype == torch.uint8 else self._held_rows(rows, "corpus", row_base)[:, :self.dim]
            return codes.float() * self._qstep[:self.dim] + self._qlo[:self.dim]
        dtype = _STORAGES[self.storage][0]
        return (rows if rows.dtype == dtype else rows.to(dtype)).float()

    @property
    def quantiser(self):
        """(lo, step) of an sq8 index: float32 [d], on the device (views of the pitch-padded arrays the kernels read)."""
        if self.storage != "sq8":
            raise AttributeError(f"storage={self.storage!r} has no quantiser")
        return self._qlo[:self.dim], self._qstep[:self.dim]

    # ---- storage="pq": the codebook, the encoder and the decoder (csrc/pq_rows.hip) ----
    @property
    def codebook(self):
        """The codebook of a pq index: float32 [M, 256, pq_dsub] on the device (what the kernels read)."""
        if self.storage != "pq":
            raise AttributeError(f"storage={self.storage!r} has no codebook")
        return self._codebook

    def _pq_set_codebook(self, corpus, dev):
        """The device codebook: the given one (held against NaN / inf here if it came on a device), or trained on the float `corpus`."""
        if self._quantiser_given is not None:
            cb = self._quantiser_given.to(dev)
            if not bool(torch.isfinite(cb).all()):
                raise ValueError("codebook must be finite")
        else:
            from .training import pq_train
            if not bool(torch.isfinite(corpus).all()):      # the trainer samples: a refusal must not depend on the sample
                bad = int(torch.nonzero(~torch.isfinite(corpus.float()).all(dim=1)).reshape(-1)[0])
                self._raise_unrepresentable(bad, self.storage, "corpus")
            cb = pq_train(corpus, self.pq_dsub)
        self._codebook = cb.contiguous()
        self._quantiser_given = None

    def _pq_encode(self, rows, what, row_base=0):
        """Float rows [n, d] (float32 / float16, unit column stride) -> their codes, uint8 [n, M], by `nlsh_pq_encode`; a row holding a
        NaN or an infinity raises ValueError naming it (`what` row `row_base` + its number)."""
        return pq_encode(rows, self._codebook, self.dim, what, row_base)

    def _pq_decode(self, codes):
        """Codes [n, >= M] (any pitch) -> the decoded rows, float32 [n, d], by `nlsh_pq_decode_rows`."""
        return pq_decode(codes, self._codebook, self.dim)

    def _pq_inv_norm(self, codes_sorted):
        """inv_norm of the sorted code rows by the float32 path's rule on the decoded rows (`nlsh_pq_inv_norm`)."""
        n, dev = int(codes_sorted.shape[0]), codes_sorted.device
        out = torch.empty((n,), dtype=torch.float32, device=dev)
        _capi.check(_capi.lib().nlsh_pq_inv_norm(_capi.ptr(codes_sorted), codes_sorted.stride(0) if n else self.row_stride, n,
                                                 _capi.ptr(self._codebook), self.pq_dsub, self.dim, _capi.ptr(out), _stream(dev)))
        return out

    def _sq8_set_quantiser(self, corpus, d, stride, dev):
        """The pitch-padded quantiser arrays (lo = 0, step = 1 behind d): the given one, or trained on `corpus` by `nlsh_sq8_train`."""
        L = _capi.lib()
        self._qlo = torch.zeros((stride,), dtype=torch.float32, device=dev)
        self._qstep = torch.ones((stride,), dtype=torch.float32, device=dev)
        if self._quantiser_given is not None:
            self._qlo[:d], self._qstep[:d] = self._quantiser_given[0].to(dev), self._quantiser_given[1].to(dev)
            return
        N = int(corpus.shape[0])
        wb = L.nlsh_sq8_train_workspace(N, d)
        if wb == 0:
            _capi.check(_capi.E_INVALID)
        ws = torch.empty((wb,), dtype=torch.uint8, device=dev)
        first_bad = torch.empty((1,), dtype=torch.int32, device=dev)
        _capi.check(L.nlsh_sq8_train(_capi.ptr(corpus), _STORE_CODE_OF_DTYPE[corpus.dtype], corpus.stride(0) if N else d, d, N, _capi.ptr(self._qlo),
                                     _capi.ptr(self._qstep), stride, _capi.ptr(first_bad), _capi.ptr(ws), wb, _stream(dev)))
        bad = int(first_bad.item())
        if bad >= 0:
            self._raise_unrepresentable(bad, self.storage, "corpus")
        wide = torch.nonzero(~torch.isfinite(self._qstep[:d])).reshape(-1)
        if wide.numel():
            raise ValueError(f"corpus column {int(wide[0])}: max - min overflows float32, no sq8 step can span it")

    def _pitch(self, d):
        """Row stride of the sorted copy, in elements: d rounded up to `row_align` (4 = 16-byte rows, the default; 32 floats = every
        float32 row starts on a 128-byte line) and to whole 16-byte units of the storage (4 / 8 / 16 elements)."""
        per16 = _STORAGES[self.storage][2]
        align = max(4, int(self.row_align))
        align = align * per16 // int(np.gcd(align, per16))
        return int((d + align - 1) // align * align)

    def _gather(self, rows, perm, out, what, row_base=0, inv_norm=None, gid=None, id_base=0):
        """Rows [*, d] (unit column stride, a dtype the library reads) picked by `perm` [M] -> `out` [M, row_stride] as the storage holds
        them, by the storage's C entry.  A compressed storage reads one pair of flags back: a row it cannot hold raises ValueError
        naming it (`what` row `row_base` + its number), the saturated rows of sq8 are counted in `last_clamped_rows`."""
        L, dev, M, d = _capi.lib(), out.device, int(perm.shape[0]), self._store_dim
        src = (_capi.ptr(rows), _STORE_CODE_OF_DTYPE[rows.dtype], rows.stride(0) if M else d, d, _capi.ptr(perm), M, _capi.ptr(out))
        tail = (_capi.ptr(inv_norm), _capi.ptr(gid), id_base)
        if not self.compressed:
            _capi.check(L.nlsh_gather_rows(src[0], *src[2:], self.row_stride, *tail, _stream(dev)))
            return
        flags = torch.zeros((2,), dtype=torch.int32, device=dev)      # first_bad (set by the call), clamped_rows (sq8 only)
        if self.storage == "sq8":
            _capi.check(L.nlsh_gather_rows_sq8(*src, self.row_stride, _capi.ptr(self._qlo), _capi.ptr(self._qstep), *tail,
                                               _capi.ptr(flags[0:1]), _capi.ptr(flags[1:2]), _stream(dev)))
        else:
            _capi.check(L.nlsh_gather_rows_typed(*src, _STORAGES[self.storage][1], self.row_stride, *tail, _capi.ptr(flags[0:1]), _stream(dev)))
        bad, clamped = flags.cpu().tolist()
        if bad >= 0:
            self._raise_unrepresentable(row_base + bad, self.storage, what)
        if self.storage == "sq8":
            self.last_clamped_rows = int(clamped)

    def _held_rows(self, rows, what, row_base=0):
        """Rows [M, d] -> the rows as a compressed index will hold them, [M, row_stride] of the storage's dtype (`_gather` in identity
        order: the library's conversion is the one statement of each storage's rule)."""
        if rows.dtype not in _STORE_CODE_OF_DTYPE:
            rows = rows.float()
        if rows.dim() != 2 or rows.stride(1) != 1:
            rows = rows.contiguous()
        M = int(rows.shape[0])
        held = torch.empty((M, self.row_stride), dtype=_STORAGES[self.storage][0], device=rows.device)
        self._gather(rows, torch.arange(M, dtype=torch.int32, device=rows.device), held, what, row_base)
        return held

    @staticmethod
    def _raise_unrepresentable(bad_row, storage, what):
        rule = ("a finite value that float16 rounds to an infinity" if storage == "float16"
                else "a NaN or an infinity" if storage in ("sq8", "pq")
                else "a value that is not an integer in [0, 255]")
        raise ValueError(f"{what} row {bad_row} holds {rule}: it cannot be stored as storage={storage!r} (nothing was changed)")

    # ------------------------------------------------------------------ build
    def _corpus_keys(self, corpus):
        """Bucket key of every corpus row, int32 [N]: `corpus_keys=` if given, else the hasher's on the rows as the index holds them."""
        N, dev = int(corpus.shape[0]), corpus.device
        if self._given_keys is not None:
            keys = self._given_keys
            if keys.shape != (N,) or keys.dtype != torch.int32 or keys.device != dev:
                raise ValueError("corpus_keys must be int32 [N] on the corpus device")
            return keys.contiguous()
        if not self.compressed:
            # indexer.py:36-38: hash(candidates, hash_times=1), in 4096-row batches when the module's mode makes batches matter
            return self.hash_device(corpus, hash_times=1)[0].view(-1)
        if N <= HASH_BATCH:
            return self.hash_device(self._dequantised(corpus), hash_times=1)[0].view(-1)
        # A compressed index hashes the dequantised rows HASH_BATCH at a time (the keys of `S.float()`, not of the caller's un-rounded
        # float32; no float32 copy of the corpus).  One probe per row is the hard key: no draw is made, so the chunks need no seeds of
        # their own.  The first call takes the hasher's next seed as the float32 build's single call does (the call counter ends where
        # that build leaves it); a BatchNorm encoder in train mode sees the same HASH_BATCH-row batches `hash_device` would cut.
        needs_train = getattr(self._hashing, "_needs_train_forward", None)
        per_batch = needs_train is not None and needs_train()
        keys = torch.empty((N, 1), dtype=torch.int32, device=dev)
        for lo in range(0, N, HASH_BATCH):
            part = self._dequantised(corpus[lo:lo + HASH_BATCH], row_base=lo)
            keys[lo:lo + HASH_BATCH] = self.hash_device(part, hash_times=1, seed=None if (lo == 0 or per_batch) else 0)[0]
        return keys.view(-1)

    def _build_index(self):
        """The CSR index and the bucket-sorted copy in the index's storage.  A compressed copy is gathered from the caller's tensor in
        its own dtype: peak extra memory is the sorted copy, the int32 arrays and O(HASH_BATCH) rows."""
        corpus = self._candidate_vectors_gpu
        if corpus.device.type != "cuda":
            raise _capi.NlshHipError(_capi.E_INVALID, "Indexer needs a device-resident corpus; there is no CPU path")
        N, d = corpus.shape
        if corpus.dtype not in (_STORE_CODE_OF_DTYPE if self.compressed else (torch.float32,)):
            corpus = corpus.float()
        if corpus.stride(1) != 1:
            corpus = corpus.contiguous()
        dev = corpus.device
        # `_store_dim`: elements of a stored row -- d, or the M code bytes of a pq row; `row_stride`: its pitch in elements
        self._store_dim = d
        if self.storage == "pq":
            d = self._pq_dim
            self._store_dim = (d + self.pq_dsub - 1) // self.pq_dsub
        self.dim, self.row_stride = d, self._pitch(self._store_dim)
        if self.storage == "pq":
            # the codebook comes first, then the codes in the caller's order: the keys are those of the DECODED rows, and the sorted copy
            # is a uint8 row store of the codes (gathered as bytes below)
            self._pq_set_codebook(corpus, dev)
            if corpus.dtype != torch.uint8:
                corpus = self._pq_encode(corpus, "corpus")
        if self.storage == "sq8":
            # the quantiser comes first: the keys are those of the DECODED rows (one read of the corpus trains it)
            self._sq8_set_quantiser(corpus, d, self.row_stride, dev)
        self.corpus_keys = self._corpus_keys(corpus)
        self.perm, self.uniq_keys, self.offsets = build_csr_device(self.corpus_keys)
        self.n_buckets = int(self.uniq_keys.shape[0])
        self.corpus_sorted = torch.empty((N, self.row_stride), dtype=_STORAGES[self.storage][0], device=dev)
        self.gid = torch.empty((N,), dtype=torch.int32, device=dev)
        self.inv_norm = torch.empty((N,), dtype=torch.float32, device=dev) if self.metric == "cosine" else None
        self._gather(corpus, self.perm, self.corpus_sorted, "corpus", inv_norm=self.inv_norm, gid=self.gid, id_base=self.id_base)
        if self.storage == "pq" and self.inv_norm is not None:      # the u8 gather took norms of the code bytes: the decoded rows' instead
            self.inv_norm = self._pq_inv_norm(self.corpus_sorted)
        if self.row_ids is not None:
            if self.row_ids.shape[0] != N or self.row_ids.dtype != torch.int32:
                raise ValueError("row_ids must be int32 [N]")
            self.gid = self.row_ids[self.perm.long()].contiguous()
        if self._given_tags is not None:      # the int64 side array in sorted order: torch plumbing, as the int32 ones
            self.tags_sorted = self._given_tags[self.perm.long()].contiguous()
            self._given_tags = None
        self._refresh_bucket_tables()

    def _refresh_bucket_tables(self):
        """What follows from `offsets` / `uniq_keys` alone: the schedule order of the buckets and the host copies of the CSR arrays."""
        L, dev = _capi.lib(), self.offsets.device
        # schedule order of the buckets (largest first) for the bucket-major scans: static per index
        self.bucket_order = torch.empty((max(self.n_buckets, 1),), dtype=torch.int32, device=dev)
        if self.n_buckets:
            ob = L.nlsh_bucket_order_workspace(self.n_buckets)
            if ob == 0:
                _capi.check(_capi.E_HIP)
            ows = torch.empty((ob,), dtype=torch.uint8, device=dev)
            _capi.check(L.nlsh_bucket_order(_capi.ptr(self.offsets), self.n_buckets, _capi.ptr(self.bucket_order), _capi.ptr(ows),
                                            ob, _stream(dev)))
        self._uniq_host = self.uniq_keys.cpu().numpy()
        self._offs_host = self.offsets.cpu().numpy().astype(np.int64)
        self.bucket_sizes = np.diff(self._offs_host)

    # ------------------------------------------------------------------ mutation
    # After any sequence of these calls every array of the index equals, word for word, what the constructor builds from the index's
    # rows in local order -- the constructor's corpus, then every added batch, minus the removed rows -- with `row_ids=` their ids and
    # `corpus_keys=` their keys.  One pass over the sorted corpus (`nlsh_csr_update`), no sort of the old keys.
    def add(self, vectors, ids=None, keys=None, tags=None) -> torch.Tensor:
        """Add float32 rows [M, d] (device; strided row views allowed; a compressed index also takes rows of its own dtype and refuses
        float32 values its storage cannot hold with a ValueError, nothing changed) -> their int32 ids (device).  `ids` (int32 [M], new and distinct)
        default to `next_id ..`; an index built with `row_ids=` has no default.  `keys` (int32 [M]) default to the hasher's keys,
        as `corpus_keys=` does in the constructor.  `tags` (int64 [M]; an index built with `tags=` only) default to 0."""
        return self.update(add=vectors, add_ids=ids, add_keys=keys, add_tags=tags)[0]

    def remove(self, ids) -> int:
        """Remove the rows with these ids (int tensor or sequence) -> how many rows went.  Unknown ids are ignored, duplicates count once."""
        return self.update(remove=ids)[1]

    def update(self, add=None, add_ids=None, add_keys=None, remove=None, add_tags=None) -> Tuple[torch.Tensor, int]:
        """`remove` and `add` in ONE pass over the corpus -> (ids of the added rows, number of rows removed).  Removal applies to the
        rows the index held before the call.  A build-path call: it runs on the current stream after the device has drained, and
        synchronises.  Out of place: the new sorted corpus is written beside the old one, which is released afterwards (peak memory:
        twice the sorted corpus).  Everything built on the old arrays -- plans, workspaces, cells, a `QueryPipeline` -- is stale
        afterwards (`generation`) -- the row tags are not: they belong to the rows and move with them (`add_tags`: int64 [M], default 0)."""
        if add_tags is not None:
            if self.tags_sorted is None:
                raise ValueError("tags= on an index built without tags: pass tags= to the constructor (nothing was changed)")
            if add is None:
                raise ValueError("add_tags without rows to add")
            add_tags = checked_tags(add_tags, int(add.shape[0]) if isinstance(add, torch.Tensor) and add.dim() == 2 else -1,
                                    self.corpus_sorted.device)
        if self.metric not in ("l2", "cosine"):
            raise NotImplementedError("update / add / remove need metric 'l2' or 'cosine': the generic-metric query reads the caller's "
                                      "corpus, which a mutated index no longer mirrors")
        if self.refine_store is not None and add_ids is not None:
            raise ValueError("add(ids=...) on an index with refine=: the refine store addresses a row by id - id_base, so added rows take "
                             "the default ids (nothing was changed)")
        dev, N = self.corpus_sorted.device, int(self.gid.shape[0])
        vectors, new_ids, new_keys = self._new_rows(add, add_ids, add_keys, dev)
        M = 0 if vectors is None else int(vectors.shape[0])
        keep, n_kept = None, N
        if remove is not None:
            rem = torch.as_tensor(remove, device=dev).reshape(-1)
            if rem.numel() and (rem.dtype.is_floating_point or rem.dtype.is_complex or rem.dtype == torch.bool):
                raise ValueError("remove must hold integer ids")
            if rem.numel() and N:
                # ~isin(gid, remove) in sorted order -- as a binary search of every gid in the SORTED removal list: `torch.isin` sorts
                # both sides, and the 10^6 gids of a SIFT1M-sized index cost it 0.4 ms per call (profiles/index_update.txt)
                rem = torch.sort(rem.long()).values
                gid64 = self.gid.long()
                keep = rem[torch.searchsorted(rem, gid64).clamp_(max=rem.numel() - 1)] != gid64
                n_kept = int(keep.sum().item())
                if n_kept == N:
                    keep = None
        if M == 0 and keep is None:
            return torch.empty((0,), dtype=torch.int32, device=dev), 0
        n_out = n_kept + M
        if n_out > 0x7FFFFFFF:
            raise ValueError(f"{n_out} rows: the index addresses its rows with int32")
        torch.cuda.synchronize(dev)         # batches in flight (other streams, pipelines) still read the arrays about to be released
        L, stride = _capi.lib(), self.row_stride
        sorted_out = torch.empty((n_out, stride), dtype=_STORAGES[self.storage][0], device=dev)
        gid_out = torch.empty((n_out,), dtype=torch.int32, device=dev)
        inv_out = torch.empty((n_out,), dtype=torch.float32, device=dev) if self.metric == "cosine" else None
        src_out = torch.empty((n_out,), dtype=torch.int32, device=dev)
        nb_cap = max(n_out, 1)
        uniq_out = torch.empty((nb_cap,), dtype=torch.int32, device=dev)
        offs_out = torch.empty((nb_cap + 1,), dtype=torch.int32, device=dev)
        nb_out = torch.zeros((1,), dtype=torch.int32, device=dev)
        ws_bytes = L.nlsh_csr_update_workspace(N, self.n_buckets, M)
        if ws_bytes == 0:
            _capi.check(_capi.E_INVALID)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        keep_u8 = None if keep is None else keep.to(torch.uint8)
        # One call: the old index | the new rows | the outputs | the workspace, with what the storage's entry adds.  Kept rows move as
        # bytes; the new rows of a compressed index arrive as it holds them (`_new_rows` has converted, checked and counted float32
        # ones), so the call converts nothing and needs no flags.  Out of place: a refusal leaves every array of the index the old one.
        code = _STORAGES[self.storage][1]
        if not self.compressed:
            entry, head, new, flags = L.nlsh_csr_update, (), (), ()
        elif self.storage == "sq8":
            entry, head, new, flags = L.nlsh_csr_update_sq8, (_capi.ptr(self._qlo), _capi.ptr(self._qstep)), (code,), (None, None)
        else:
            entry, head, new, flags = L.nlsh_csr_update_typed, (code,), (_STORE_CODE_OF_DTYPE[vectors.dtype] if M else code,), (None,)
        _capi.check(entry(
            _capi.ptr(self.corpus_sorted), *head, stride, self._store_dim, _capi.ptr(self.gid), _capi.ptr(self.inv_norm), _capi.ptr(self.uniq_keys),
            _capi.ptr(self.offsets), N, self.n_buckets, _capi.ptr(keep_u8), n_kept,
            _capi.ptr(vectors), *new, vectors.stride(0) if M else self._store_dim, _capi.ptr(new_keys), _capi.ptr(new_ids), M,
            _capi.ptr(sorted_out), stride, _capi.ptr(gid_out), _capi.ptr(inv_out), _capi.ptr(src_out), _capi.ptr(uniq_out), _capi.ptr(offs_out),
            _capi.ptr(nb_out), *flags, _capi.ptr(ws), ws_bytes, _stream(dev)))
        n_buckets = int(nb_out.item())
        if self.storage == "pq" and inv_out is not None and n_out:      # as in the build: the norms of the decoded rows
            inv_out = self._pq_inv_norm(sorted_out)
        # the int32 side arrays in LOCAL order, from where every sorted row came from (`src_out`): torch plumbing, 4 bytes per row
        src = src_out.long()
        if N:
            local = self.perm.long()
            keep_local = None
            if keep is not None:
                keep_local = torch.empty((N,), dtype=torch.bool, device=dev)
                keep_local[local] = keep
                local = (torch.cumsum(keep_local, 0) - 1)[local]        # new local row of the old row at each old sorted position
            perm = torch.where(src >= 0, local[src.clamp(min=0)], n_kept + ~src)
            old_keys = self.corpus_keys if keep_local is None else self.corpus_keys[keep_local]
            old_ids = None if self.row_ids is None else (self.row_ids if keep_local is None else self.row_ids[keep_local])
        else:
            perm, old_keys = ~src, self.corpus_keys
            old_ids = None if self.row_ids is None else self.row_ids
        if self.tags_sorted is not None:
            # the tags follow the rows through `src_out`, as the keys and ids do through `perm`: a kept row's from its old sorted position,
            # a new row's from `add_tags` (default 0)
            new_tags = add_tags if add_tags is not None else torch.zeros((M,), dtype=torch.int64, device=dev)
            if M == 0:
                self.tags_sorted = self.tags_sorted[src]
            elif N == 0:
                self.tags_sorted = new_tags[~src]
            else:
                self.tags_sorted = torch.where(src >= 0, self.tags_sorted[src.clamp(min=0)], new_tags[(~src).clamp(min=0)])
        self.perm = perm.to(torch.int32)
        self.corpus_keys = torch.cat([old_keys, new_keys]) if M else old_keys.contiguous()
        if self.row_ids is not None:
            self.row_ids = torch.cat([old_ids, new_ids]) if M else old_ids.contiguous()
        self.corpus_sorted, self.gid, self.inv_norm = sorted_out, gid_out, inv_out
        self.uniq_keys, self.offsets, self.n_buckets = uniq_out[:n_buckets], offs_out[:n_buckets + 1], n_buckets
        self._refresh_bucket_tables()
        if M:
            self.next_id = max(self.next_id, int(new_ids.max().item()) + 1)
        self._drop_derived()
        self._candidate_vectors_gpu = None      # the index owns its rows now
        if M and self.refine_store is not None:
            # the caller's rows as they came, under the ids they were given (default ids: next_id .. = id_base + rows of the store);
            # `remove` leaves the store alone -- stage one can no longer return a removed id
            originals = add
            if self.storage in ("sq8", "pq") and add.dtype == torch.uint8:
                originals = self._dequantised(vectors)
            assert int(new_ids[0].item()) == self.id_base + self.refine_store.n_rows
            self.refine_store.append(originals)
        self.generation += 1
        return (new_ids if M else torch.empty((0,), dtype=torch.int32, device=dev)), N - n_kept

    def _new_rows(self, add, add_ids, add_keys, dev):
        """`update`'s new rows, checked before anything changes -> (vectors fp32 [M, d] unit column stride, ids int32 [M], keys int32 [M]),
        all None for no rows."""
        if add is None:
            if add_ids is not None or add_keys is not None:
                raise ValueError("add_ids / add_keys without rows to add")
            return None, None, None
        if not isinstance(add, torch.Tensor) or add.device.type != "cuda":
            raise _capi.NlshHipError(_capi.E_INVALID, "added rows must be a device-resident tensor; there is no CPU path")
        if add.device != dev:
            raise ValueError(f"added rows are on {add.device}, the index on {dev}")
        width = self._store_dim if (self.storage == "pq" and isinstance(add, torch.Tensor) and add.dtype == torch.uint8) else self.dim
        if add.dim() != 2 or add.shape[1] != width:
            raise ValueError(f"added rows must be [M, {width}], got {tuple(add.shape)}")
        if add.dtype != torch.float32 and not (self.compressed and add.dtype == _STORAGES[self.storage][0]):
            own = "uint8 (codes)" if self.storage in ("sq8", "pq") else self.storage
            raise ValueError(f"added rows must be float32{' or ' + own if self.compressed else ''}, got {add.dtype}")
        M = int(add.shape[0])
        if M == 0:
            return None, None, None
        vectors = add if add.stride(1) == 1 else add.contiguous()
        if self.compressed:
            # float32 rows are converted and checked FIRST, by the storage's own rule (sq8 saturates: `last_clamped_rows`): a refusal comes
            # before the hasher is touched, and what is hashed and merged below is the rows as the index will hold them.  Rows of the
            # storage's own dtype are held as they are (uint8 rows of an sq8 index are codes).
            if self.storage == "sq8":
                self.last_clamped_rows = 0
            if vectors.dtype == torch.float32:
                vectors = self._pq_encode(vectors, "added") if self.storage == "pq" else self._held_rows(vectors, "added")[:, :self.dim]
        if add_keys is not None:
            keys = add_keys
            if not isinstance(keys, torch.Tensor) or keys.shape != (M,) or keys.dtype != torch.int32 or keys.device != dev:
                raise ValueError("keys must be int32 [M] on the index's device")
            keys = keys.contiguous()
        else:
            needs_train = getattr(self._hashing, "_needs_train_forward", None)
            if needs_train is not None and needs_train():
                raise _capi.NlshHipError(_capi.E_UNSUPPORTED, "add() needs eval mode for BatchNorm encoders (train_mode(False)): batch statistics "
                                                              "would make a row's key depend on the batch it arrived in; or pass keys=")
            # the call `_build_index` makes (a compressed index hashes the rows as it will hold them)
            keys = self.hash_device(self._dequantised(vectors) if self.compressed else vectors, hash_times=1)[0].reshape(-1).contiguous()
        if add_ids is None:
            if self.row_ids is not None:
                raise ValueError("an index built with row_ids= has no default ids: pass ids=")
            if self.next_id + M - 1 > 0x7FFFFFFF:
                raise ValueError("row ids are int32: next_id + M exceeds 2^31 - 1")
            ids = torch.arange(self.next_id, self.next_id + M, dtype=torch.int32, device=dev)
        else:
            ids = torch.as_tensor(add_ids, device=dev)
            if ids.shape != (M,) or ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
                raise ValueError("ids must be M integers")
            if ids.dtype != torch.int32:
                if int(ids.min().item()) < -(1 << 31) or int(ids.max().item()) > 0x7FFFFFFF:
                    raise ValueError("row ids are int32")
                ids = ids.to(torch.int32)
            ids = ids.contiguous()
            if int(torch.unique(ids).numel()) != M:
                raise ValueError("ids must be distinct")
            if bool(torch.isin(ids, self.gid).any().item()):
                raise ValueError("ids must be new: some are in the index already")
        return vectors, ids, keys

    def _drop_derived(self):
        """Everything derived from the index arrays of the previous generation.  The kept range plans hold raw pointers (a new tensor
        can land on an old address, so an equal `data_ptr` proves nothing) and the bucket-major PLAN phase keeps one counter per
        bucket at the head of each workspace -- `n_buckets` has changed."""
        self._cells = {}
        self._index2row = None
        self._perm_host = None
        self._e_sb = None
        self._ws = {}
        self._max_tasks = {}
        for name in ("_range_plans", "_ranked_key_tables", "_key_tables", "_held", "_bucket_dir"):
            self.__dict__.pop(name, None)

    # ------------------------------------------------------------------ row tags
    def set_tags(self, ids, tags) -> int:
        """Change the tags of held rows in place: `ids` (integer tensor or sequence), `tags` (int64, one per id) -> how many rows were
        found.  Unknown ids are ignored, as in `remove`; of a repeated id one of its tags wins.  No row moves and `generation` stays:
        RowFilters, plans and workspaces remain valid, and the next call sees the new tags (stream order)."""
        if self.tags_sorted is None:
            raise ValueError("set_tags on an index built without tags: pass tags= to the constructor")
        dev = self.tags_sorted.device
        ids = torch.as_tensor(ids, device=dev).reshape(-1)
        if ids.numel() and (ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool):
            raise ValueError("ids must hold integer ids")
        tags = checked_tags(tags if isinstance(tags, torch.Tensor) else torch.as_tensor(tags, dtype=torch.int64, device=dev).reshape(-1),
                            int(ids.numel()), dev)
        if ids.numel() == 0 or self.gid.numel() == 0:
            return 0
        sorted_gid, order = torch.sort(self.gid.long())
        ids = ids.long()
        pos = torch.searchsorted(sorted_gid, ids).clamp_(max=sorted_gid.numel() - 1)
        found = sorted_gid[pos] == ids
        rows = order[pos[found]]
        self.tags_sorted[rows] = tags[found]
        return int(torch.unique(rows).numel())

    def tags_local(self) -> torch.Tensor:
        """The tags in LOCAL row order (int64 [N]; the constructor's rows, then every added batch, minus the removed rows): what
        `Indexer(..., tags=)` takes to rebuild this index."""
        if self.tags_sorted is None:
            raise ValueError("an index built without tags has none")
        out = torch.empty_like(self.tags_sorted)
        out[self.perm.long()] = self.tags_sorted
        return out

    # ------------------------------------------------------------------ row filters
    def row_filter(self, allow=None, deny=None, mask=None) -> RowFilter:
        """A per-call row filter of this index (`filter=` of `scan_tensors` / `query_tensors` / `query_with_keys` / `query`): EXACTLY ONE
        of `allow` (only rows with these ids may be returned), `deny` (every row but these) and `mask` (a bool or uint8 DEVICE tensor
        indexed by `id - id_base`, non-zero = allowed; ids outside it are denied).  `allow` / `deny` hold integer ids, as a tensor or a
        sequence; unknown ids are ignored and duplicates count once, as in `remove` (they are sorted and de-duplicated here).  The
        bitset is built on the device (`nlsh_row_filter_build`, one pass over the row ids); the call synchronises to read
        `n_allowed`.  The filter is this index's, in this `generation`: after an effective `add` / `remove` / `update` it is stale
        and a call that is given it raises ValueError -- build a new one."""
        if (allow is not None) + (deny is not None) + (mask is not None) != 1:
            raise ValueError("row_filter takes exactly one of allow=, deny= and mask=")
        if self.metric not in ("l2", "cosine"):
            raise NotImplementedError("row filters need metric 'l2' or 'cosine': the filter is read by the tiled scan kernel")
        ids = None
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 1:
                raise ValueError("mask must be a 1-d bool or uint8 tensor indexed by id - id_base")
            if mask.device.type != "cuda":
                raise _capi.NlshHipError(_capi.E_INVALID, "mask must be device-resident; there is no CPU path")
        else:
            given = allow if allow is not None else deny
            name = "allow" if allow is not None else "deny"
            if isinstance(given, torch.Tensor):
                ids = given
                if ids.numel() and (ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool):
                    raise ValueError(f"{name} must hold integer ids")
            else:
                arr = np.asarray(list(given))
                if arr.size and arr.dtype.kind not in "iu":
                    raise ValueError(f"{name} must hold integer ids")
                ids = torch.as_tensor(arr.astype(np.int64).reshape(-1))
        dev, N = self.gid.device, int(self.gid.shape[0])
        L = _capi.lib()
        words = torch.empty((L.nlsh_row_filter_words(N),), dtype=torch.int32, device=dev)
        n_allowed = torch.empty((1,), dtype=torch.int32, device=dev)
        if ids is not None:
            ids = ids.to(dev).reshape(-1).long()
            ids = torch.unique(ids[(ids >= -(1 << 31)) & (ids <= 0x7FFFFFFF)]).to(torch.int32)      # ascending, distinct; no row has an id outside int32
            src = ids if ids.numel() else torch.zeros((1,), dtype=torch.int32, device=dev)          # the empty list still names its source
            args = (src.data_ptr(), int(ids.numel()), None, 0, 0)
        else:
            if mask.device != dev:
                raise ValueError(f"mask is on {mask.device}, the index on {dev}")
            src = mask.contiguous().view(torch.uint8)
            n_dense = int(src.numel())
            if n_dense == 0:
                src = torch.zeros((1,), dtype=torch.uint8, device=dev)
            args = (None, 0, src.data_ptr(), n_dense, self.id_base)
        _capi.check(L.nlsh_row_filter_build(self.gid.data_ptr() if N else None, N, *args, int(deny is not None),
                                            words.data_ptr() if N else None, n_allowed.data_ptr(), _stream(dev)))
        return RowFilter(self, words, int(n_allowed.item()), self.generation)

    def _checked_filter(self, filter, algo=None, tag_mask=None, tag_match="any", query_vectors=None):
        """`filter=` / `tag_mask=` / `tag_match=` of a call, checked before anything is launched -> None, the RowFilter, or -- a tagged
        call -- the TagFilter that carries masks, mode and RowFilter along the routes a RowFilter takes."""
        if isinstance(filter, TagFilter):       # a call of this class handing its checked TagFilter on
            return filter
        if tag_match not in TAG_MATCH:
            raise ValueError(f"tag_match must be one of {tuple(TAG_MATCH)}, got {tag_match!r}")
        if tag_mask is not None:
            if self.storage == "pq":
                raise NotImplementedError("tag_mask= is not built for storage='pq': the tagged kernels read no codebook (DESIGN.md 7)")
            if self.tags_sorted is None:
                raise ValueError("tag_mask= on an index built without tags: pass tags= to the constructor")
            if isinstance(tag_mask, torch.Tensor):
                n_queries = None if query_vectors is None else int(query_vectors.shape[0])
                if tag_mask.dtype != torch.int64 or tag_mask.dim() != 1 or (n_queries is not None and tag_mask.shape[0] != n_queries):
                    raise ValueError(f"tag_mask must be one Python int or an int64 tensor with one mask per query"
                                     f"{'' if n_queries is None else f' ({n_queries},)'}, got {tag_mask.dtype} {tuple(tag_mask.shape)}")
                if tag_mask.device != self.tags_sorted.device:
                    raise ValueError(f"tag_mask is on {tag_mask.device}, the index on {self.tags_sorted.device}")
                tag_mask = tag_mask.contiguous()
            elif isinstance(tag_mask, bool) or not isinstance(tag_mask, numbers.Integral):
                raise ValueError(f"tag_mask must be one Python int or an int64 tensor with one mask per query, got {type(tag_mask).__name__}")
            else:
                tag_mask = int(tag_mask)
                if not -(1 << 63) <= tag_mask < (1 << 64):
                    raise ValueError(f"tag_mask={tag_mask} does not fit 64 bits")
                tag_mask = tag_mask - (1 << 64) if tag_mask >= (1 << 63) else tag_mask     # the same 64 bits in the signed container
            if self.metric not in ("l2", "cosine"):
                raise NotImplementedError("tag_mask= needs metric 'l2' or 'cosine': the tags are read by the tiled scan kernel")
            if self.algo in ("query", "bucket") or algo in (_capi.SCAN_QUERY_MAJOR, _capi.SCAN_BUCKET_MAJOR):
                raise ValueError("a tagged call (tag_mask=) is scanned by the tiled schedule only: algo='query' / 'bucket' cannot read row "
                                 "tags (algo=None or 'tiled')")
            return TagFilter(tag_mask, TAG_MATCH[tag_match], self._checked_filter(filter, algo))
        if filter is None:
            return None
        if not isinstance(filter, RowFilter):
            raise ValueError(f"filter must be None or a RowFilter built by this index's row_filter(), got {type(filter).__name__}")
        if filter._index() is not self:
            raise ValueError("filter was built by another index: a RowFilter addresses the sorted rows of the index that built it")
        if filter.generation != self.generation:
            raise ValueError(f"stale filter: built at generation {filter.generation}, the index is at {self.generation} "
                             "(add / remove / update move rows); build a new one with row_filter()")
        if self.metric not in ("l2", "cosine"):
            raise NotImplementedError("filter= needs metric 'l2' or 'cosine': the filter is read by the tiled scan kernel")
        if self.algo in ("query", "bucket") or algo in (_capi.SCAN_QUERY_MAJOR, _capi.SCAN_BUCKET_MAJOR):
            raise ValueError("a filtered call is scanned by the tiled schedule only: algo='query' / 'bucket' cannot read a row filter "
                             "(algo=None or 'tiled')")
        return filter

    @property
    def index2row(self) -> Dict[int, torch.Tensor]:
        """Reference attribute (indexer.py:38; read by trainers/base.py:87-89): materialised lazily
        as views of one int64 copy of `perm`."""
        if self._index2row is None:
            rows = self.gid.long()
            names = self._uniq_host.astype(np.int64)
            if self._hashing.key_mode == _capi.KEY_FULL:
                names = names & 0xFFFFFFFF
            self._index2row = {int(k): v for k, v in zip(names.tolist(), torch.split(rows, self.bucket_sizes.tolist()))}
        return self._index2row

    def bucket_stats(self):
        s = self.bucket_sizes
        if len(s) == 0:
            return {"n_indexes": 0, "mean": 0.0, "median": 0.0, "max": 0, "std_index_rows": 0.0}
        return {"n_indexes": int(len(s)), "mean": float(s.mean()), "median": float(np.median(s)), "max": int(s.max()),
                "std_index_rows": float(s.std())}

    # ------------------------------------------------------------------ hashing
    def _n_multi_rows(self, n, batch_size=HASH_BATCH):
        # indexer.py:43-53: only full batches get hash_times; the trailing partial batch is n=1 (F6)
        return (n // batch_size) * batch_size if self.compat else n

    @contextlib.contextmanager
    def _probe_mode(self, probes):
        """A call's `probes=` keyword ("sampled" | "ranked"): the hasher's `probes` attribute is set for the duration of the call and
        restored on every exit.  Anything else is a ValueError before the call does anything.  (Callers skip this for None: the
        hasher is left as it is and the default path pays nothing.)"""
        mode = _capi.probe_mode(probes)
        h = self._hashing
        old = getattr(h, "probes", "sampled")
        h.probes = mode
        try:
            yield
        finally:
            h.probes = old

    def _candidate_budget(self, candidate_budget, probes):
        """A call's `candidate_budget=` keyword, checked before the call does anything: an integer >= 1, the ranked mode (the call's
        `probes=` or the hasher's attribute) and a device metric.  -> the int32 the kernel takes (a row holds fewer than 2^31
        candidates, so anything above INT32_MAX is INT32_MAX)."""
        mode = _capi.probe_mode(probes, getattr(self._hashing, "probes", "sampled"))
        if isinstance(candidate_budget, bool) or not isinstance(candidate_budget, numbers.Integral):
            raise ValueError(f"candidate_budget must be None or an integer >= 1, got {candidate_budget!r}")
        if candidate_budget < 1:
            raise ValueError(f"candidate_budget must be >= 1, got {candidate_budget}")
        if mode != "ranked":
            raise ValueError("candidate_budget needs the ranked probe mode (probes='ranked' on the call or a ranked hasher): "
                             "sampled draws come in no order to cut")
        if self.metric not in ("l2", "cosine"):
            raise NotImplementedError("candidate_budget needs metric 'l2' or 'cosine' (use SIFT.distance / Glove.distance)")
        return min(int(candidate_budget), 0x7FFFFFFF)

    def _hash_budget(self, query_vectors, batch_size, hash_times, budget, out=None):
        """Ranked keys cut at a candidate budget -> (keys, nkeys, ncand): the hasher's one-probe encode for z and the hard code, then
        `nlsh_probe_ranked_budget` on this index's CSR arrays; `hash_times` is the cap."""
        if hash_times < 1:
            raise ValueError(f"`n` should be positive integer, but got {hash_times}")
        if hash_times > _capi.MAX_ENCODE_PROBES:
            raise _capi.NlshHipError(_capi.E_UNSUPPORTED, f"hash_times={hash_times} > {_capi.MAX_ENCODE_PROBES}")
        h = self._hashing
        q = self._as_queries(query_vectors)
        if hasattr(h, "hash_budget_device"):    # a family that ranks its own keys (Categorical: bins, not bit codes)
            return h.hash_budget_device(q, hash_times, self._n_multi_rows(q.shape[0], batch_size), self.uniq_keys, self.offsets,
                                        self.n_buckets, budget, out=out)
        z, code = h.encode_device(q)
        B, H, dev = q.shape[0], z.shape[1], q.device
        if out is not None:
            keys, nkeys = out
            if keys.shape != (B, hash_times) or keys.dtype != torch.int32 or nkeys.shape != (B,) or nkeys.dtype != torch.int32:
                raise ValueError("out must be (int32 [B, n], int32 [B])")
        else:
            keys = torch.empty((B, hash_times), dtype=torch.int32, device=dev)
            nkeys = torch.empty((B,), dtype=torch.int32, device=dev)
        ncand = torch.empty((B,), dtype=torch.int32, device=dev)
        _capi.check(_capi.lib().nlsh_probe_ranked_budget(
            _capi.ptr(z), z.stride(0) if B else H, _capi.ptr(code), B, H, h.key_mode, hash_times, self._n_multi_rows(B, batch_size),
            _capi.ptr(self.uniq_keys), _capi.ptr(self.offsets), self.n_buckets, budget, _capi.ptr(keys), _capi.ptr(nkeys), None,
            _capi.ptr(ncand), _stream(dev)))
        return keys, nkeys, ncand

    def hash_device(self, query_vectors, batch_size=HASH_BATCH, hash_times=1, seed=None, out=None, probes=None, candidate_budget=None):
        """`candidate_budget` (ranked mode only; None = off): every query stops probing after the first key that brings its candidates
        to the budget, `hash_times` is the cap (include/nlsh_hip.h, nlsh_probe_ranked_budget)."""
        if candidate_budget is not None:
            return self._hash_budget(query_vectors, batch_size, hash_times, self._candidate_budget(candidate_budget, probes), out)[:2]
        if probes is None:
            return self._hash_device(query_vectors, batch_size, hash_times, seed, out)
        with self._probe_mode(probes):
            return self._hash_device(query_vectors, batch_size, hash_times, seed, out)

    def _hash_device(self, query_vectors, batch_size=HASH_BATCH, hash_times=1, seed=None, out=None):
        needs_train = getattr(self._hashing, "_needs_train_forward", None)
        if needs_train is not None and needs_train() and query_vectors.shape[0] > batch_size:
            # BatchNorm encoder in TRAIN mode: the reference feeds the module `batch_size`-row batches (nlsh/indexer.py:40-53), so the
            # batch statistics -- and the running-statistics updates -- are per batch, the trailing partial batch on its own
            # statistics with n = 1 (F6).  One forward over all rows would use other statistics and hold every activation at once.
            n, parts = query_vectors.shape[0], []
            full = (n // batch_size) * batch_size
            for lo in range(0, full, batch_size):
                parts.append(self._hashing.hash_device(query_vectors[lo:lo + batch_size], n=hash_times, seed=seed))
            if full < n:
                tail_n = 1 if self.compat else hash_times
                tk, tn = self._hashing.hash_device(query_vectors[full:], n=tail_n, seed=seed)
                if tk.shape[1] < hash_times:
                    tk = torch.nn.functional.pad(tk, (0, hash_times - tk.shape[1]))
                parts.append((tk, tn))
            keys, nkeys = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
            if out is not None:
                out[0].copy_(keys)
                out[1].copy_(nkeys)
                keys, nkeys = out
            return keys, nkeys
        return self._hashing.hash_device(query_vectors, n=hash_times,
                                         n_multi_rows=self._n_multi_rows(query_vectors.shape[0], batch_size), seed=seed, out=out)

    def hash(self, query_vectors, batch_size=HASH_BATCH, hash_times=1, probes=None, candidate_budget=None) -> List[Set[int]]:
        keys, nkeys = self.hash_device(query_vectors, batch_size, hash_times, probes=probes, candidate_budget=candidate_budget)
        return keys_to_sets(keys, nkeys, self._hashing.key_mode)

    # ------------------------------------------------------------------ query
    def _size_biased_bucket(self):
        if self._e_sb is None:                                       # static per index; every batch asks for it
            s = self.bucket_sizes.astype(np.float64)
            n = max(float(s.sum()), 1.0)
            self._e_sb = float((s * s).sum() / n) if len(s) else 0.0  # expected size of the bucket a point lands in
        return self._e_sb

    def choose_algo(self, Q, P):
        """The LDS-tiled bucket-major schedule from 64 (query, probe) pairs per batch on, the query-major stream below that.

        r04, with small buckets sharing 64-row windows (`choose_window`), tools/scan_bench.py --queries Q --algo ..., scan kernel /
        whole device step in ms on one box (profiles/r04_algo_by_batch_size.txt):
                            Q = 1          16           200          1000         2500         5000         10000
            GloVe   tiled   .011 / .113   .013 / .082   .017 / .082  .038 / .101  .068 / .135  .095 / .168  .123 / .22
                    query   .043 / .093   .044 / .104   .050 / .135  .057 / .143  .071 / .158  .114 / .203  .237 (r03)
            SIFT1M  tiled   .014 / .074   .014 / .074   .020 / .074  .051 / .104  .075 / .131  .163 / .222  .24
                    query   .031 / .067   .046 / .080   .054 / .092  .069 / .108  .146 / .189  .846 / .924  1.65 (r01)
        (the SURVEY-generator SIFT1M index behaves like GloVe; the wave-level bucket-major schedule, algo="bucket", lost every cell of
        this table by 2-4x and is only reachable by name).  r03's rule sent balanced hashes with tiny buckets and small batches to the
        query-major stream because a task per (bucket, query group) cost ~9 us of latency per pair; windows removed that.  Only a
        batch of a handful of queries still prefers the query-major schedule's shorter PLAN phase (one kernel instead of four).
        The rule depends on the batch shape alone, so every shard count picks the same arithmetic (`schedule_stats` is kept for the
        sharded builds' interface and no longer enters)."""
        if self.compressed:         # float16 / uint8 rows are read by the tiled schedule only, whatever the batch shape
            return _capi.SCAN_BUCKET_TILED
        if self.algo is not None:
            return {"query": _capi.SCAN_QUERY_MAJOR, "bucket": _capi.SCAN_BUCKET_MAJOR, "tiled": _capi.SCAN_BUCKET_TILED}[self.algo]
        return _capi.SCAN_BUCKET_TILED if Q * P >= 64 else _capi.SCAN_QUERY_MAJOR

    def cells(self, window_rows):
        """(cell_of, cell_offsets, cell_order, n_cells) of this index for one window size: `nlsh_build_cells`, once per (index, size)."""
        got = self._cells.get(window_rows)
        if got is None:
            L = _capi.lib()
            dev, nb = self.offsets.device, self.n_buckets
            cell_of = torch.empty((max(nb, 1),), dtype=torch.int32, device=dev)
            cell_offsets = torch.empty((nb + 1,), dtype=torch.int32, device=dev)
            cell_order = torch.empty((max(nb, 1),), dtype=torch.int32, device=dev)
            n_cells = torch.zeros((1,), dtype=torch.int32, device=dev)
            wb = L.nlsh_build_cells_workspace(nb)
            if wb == 0 and nb:
                _capi.check(_capi.E_HIP)
            ws = torch.empty((max(wb, 1),), dtype=torch.uint8, device=dev)
            _capi.check(L.nlsh_build_cells(_capi.ptr(self.offsets), nb, window_rows, _capi.ptr(cell_of), _capi.ptr(cell_offsets),
                                           _capi.ptr(cell_order), _capi.ptr(n_cells), _capi.ptr(ws), wb, _stream(dev)))
            nc = int(n_cells.item())    # like the bucket count of the index build: once per index, not on the query path
            got = self._cells[window_rows] = (cell_of, cell_offsets[:nc + 1], cell_order[:max(nc, 1)], nc)
        return got

    def _cells_or_buckets(self, window):
        """(cell_of, cell_offsets, order, n_cells) as a launch takes them: the cells of a row window, or -- window 0 -- none of them and
        the buckets in `bucket_order`."""
        return self.cells(window) if window else (None, None, self.bucket_order, 0)

    def choose_window(self, Q, P, algo):
        """Row window of the small-bucket packing for one batch shape (tiled schedule only): 64 rows unless forced.
        Measured (r04, tools/scan_bench.py --window 0,64,128,256 --rounds 4, same process and keys, scan kernel ms, one box):
            window            0       64      128     256
            SIFT1M headline   0.2427  0.2400  0.2434  0.2522     (skewed 16-bit hash, 45 k pairs on 5.1 k probed buckets)
            SIFT1M clusters   0.1613  0.1359  0.1377  0.1575     (SURVEY 8(d) generator, 49.7 k pairs on 18.1 k buckets)
            GloVe-1.2M        0.1588  0.1231  0.1244  0.1497     (24-bit cosine, 64.7 k pairs on 36.6 k buckets)
        A 64-row window adds no arithmetic (a lone small bucket already pays a whole 64-row tile and the fat single-tile stages)
        and only merges tasks; wider windows score every row of the window for every query of the task, which the balanced
        workloads earn back in task count up to 128 rows and the skewed headline does not.  One value keeps every shard count on
        the same arithmetic-free choice (results never depend on it)."""
        if algo != _capi.SCAN_BUCKET_TILED or self.n_buckets == 0:
            return 0
        if self.window_rows is not None:
            return self.window_rows
        return 64

    def _tkey(self, algo, Q, P):
        """Key of a batch shape's task table in `_max_tasks`: (schedule, Q, P, row window of the small-bucket packing)."""
        return (algo, Q, P, self.choose_window(Q, P, algo))

    def _estimate_tasks(self, Q, P, seg, algo):
        biased = self._size_biased_bucket()
        if algo == _capi.SCAN_BUCKET_TILED:   # tasks = (256-row segment, <= 16 queries)
            est = Q * min(P, 4) * (1.0 / 16 + biased / 256 / 16) + self.n_buckets
        elif algo == _capi.SCAN_BUCKET_MAJOR:
            est = Q * min(P, 4) * (1.0 / 4 + biased / seg / 4) + self.n_buckets
        else:
            est = Q * (1.0 + min(P, 4) * biased / seg)
        return int(min(max(1.5 * est + 1024, Q + 1024), 2 ** 31 - 8))

    def _task_table(self, algo, Q, P):
        """(tkey, window, max_tasks) of a batch shape -- the only place that consults or seeds `_max_tasks` for one.  The task table is
        sized per (schedule, batch shape): a larger batch after a smaller one re-estimates instead of reusing a table that `check=False`
        callers would silently overflow; a smaller one takes the smallest table of the same schedule and window that served a batch at
        least as large."""
        tkey = self._tkey(algo, Q, P)
        window = tkey[3]
        max_tasks = self._max_tasks.get(tkey)
        if max_tasks is None:
            grown = [v for (a_, q_, p_, w_), v in self._max_tasks.items() if a_ == algo and q_ >= Q and p_ >= P and w_ == window]
            max_tasks = self._max_tasks[tkey] = min(grown) if grown else self._estimate_tasks(Q, P, self.seg_rows or 512, algo)
        return tkey, window, max_tasks

    def _workspace(self, dev, stream, bucket_major, ws_bytes):
        """(wkey, ws): one workspace per stream and schedule family, fetched or zero-allocated -- the bucket-major PLAN phase keeps its
        per-bucket counters at the head of the workspace ZERO between calls (include/nlsh_hip.h), so nothing else may write there."""
        wkey = (stream, bucket_major)
        ws = self._ws.get(wkey)
        if ws is None or ws.numel() < ws_bytes or ws.device != dev:
            ws = self._ws[wkey] = torch.zeros((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
        return wkey, ws

    @staticmethod
    def _outputs(Q, k, dev, want_keys=False):
        """One batch's outputs: (out_dist, pack, out_idx, ncand, status, out_keys | None).  ids, candidate counts and the two status
        words share ONE int32 buffer (`pack`): `query()` brings all three to the host with a single copy (and a single
        synchronisation) instead of four."""
        out_dist = torch.empty((Q, k), dtype=torch.float32, device=dev)
        pack = torch.empty((Q * k + Q + 2,), dtype=torch.int32, device=dev)
        out_keys = torch.empty((Q, k), dtype=torch.int64, device=dev) if want_keys else None
        out_idx, ncand, status = pack.split((Q * k, Q, 2))
        return out_dist, pack, out_idx.view(Q, k), ncand, status, out_keys

    def _set_last(self, status, algo, window, pack, tkey, max_tasks):
        """What the last launch ran with (`max_tasks`: its table, before any trim); bench.py, the tests and the tools read these."""
        self.last_status = status
        self.last_algo, self.last_window = algo, window
        self._last_pack, self._last_tkey, self._last_max_tasks = pack, tkey, max_tasks

    def _refine_k1(self, k, refine_k):
        """Stage one's k of a call on this index: 0 = no second stage (no store, or `refine_k=0`); host arithmetic and refusals only."""
        if self.refine_store is None:
            if refine_k:
                raise ValueError("refine_k= needs an index built with refine='device' or 'host'")
            return 0
        return stage_one_k(k, self.refine_factor, refine_k)

    def _refuse_refine(self, what):
        if self.refine is not None:
            raise NotImplementedError(f"{what} is not built for an index with refine=: the re-rank is a top-k stage (DESIGN.md 7)")

    @staticmethod
    def _refuse_tags(what, tag_mask):
        if tag_mask is not None:
            raise NotImplementedError(f"{what} takes no tag_mask: per-query tag filters are built for the top-k calls (DESIGN.md 7)")

    def _rerank(self, query_vectors, stage_one, k, want_keys, check=True):
        """Stage two behind a stage-one result (dist, idx [Q, k1], ncand, ...): ONE further launch on the same stream, stage one's idx its
        candidate table, nothing read on the host in between -> (exact dist [Q, k], idx [Q, k], stage one's ncand, stage two's keys64 | None)."""
        out = self.refine_store.rerank(self._as_queries(query_vectors), stage_one[1], k, want_keys=True, check=check)
        path = self.last_query_path or "two_step"        # (a bare `scan_tensors` call is the two-step route's second step)
        self.last_query_path = path if path.endswith("+refine") else path + "+refine"
        return out[0], out[1], stage_one[2], out[3] if want_keys else None

    def scan_tensors(self, query_vectors, keys, nkeys, k=10, want_keys=False, check=True, events=None, algo=None, filter=None, refine_k=None,
                     tag_mask=None, tag_match="any"):
        """Scan stage on a device key table -> (dist [Q,k], idx [Q,k], ncand [Q], keys64 | None).
        tag_mask (an index built with `tags=` only; None = off): one Python int (every query's mask) or an int64 [Q] device tensor, matched
        against the rows' 64-bit tags by `tag_match` -- "any": (tag & mask) != 0, "all": (tag & mask) == mask, "eq": tag == mask.  Query
        q's result is, word for word, that of the index built from the rows that pass ITS mask alone, as with `filter=`; with `filter=`
        as well a row must pass both.  `ncand` counts bucket rows before the tags.  Tiled schedule.
        filter (a `RowFilter` of this index, `row_filter()`; None = off): the result is, word for word, that of the index built from the
        allowed rows alone (same ids, same bucket keys, same key table) -- ids, distance bits and keys64, with -1 / +inf / ~0 behind a
        list shorter than k.  `ncand` stays the rows of the probed buckets, counted BEFORE the filter: the work the scan did, equal to
        the unfiltered call's.  A filtered call takes the tiled schedule whatever the batch shape, as a compressed index does."""
        filter = self._checked_filter(filter, algo, tag_mask, tag_match, query_vectors)
        k1 = self._refine_k1(k, refine_k)
        if k1:      # stage one at k1 (this call, unrefined), then the re-rank
            one = self.scan_tensors(query_vectors, keys, nkeys, k=k1, check=check, events=events, algo=algo, filter=filter, refine_k=0)
            return self._rerank(query_vectors, one, k, want_keys, check)
        if self.metric not in ("l2", "cosine"):
            raise NotImplementedError("fused scan needs metric 'l2' or 'cosine' (use SIFT.distance / Glove.distance)")
        q = self._as_queries(query_vectors)
        Q, d = q.shape
        if d != self.dim:
            raise ValueError(f"query dim {d} != corpus dim {self.dim}")
        dev = q.device
        if keys.shape[1] > _capi.MAX_PROBES:
            return self._scan_sliced(q, keys, nkeys, k, want_keys, check, filter)
        keys = keys.contiguous()
        nkeys = nkeys.contiguous()
        P = keys.shape[1]
        out_dist, pack, out_idx, ncand, status, out_keys = self._outputs(Q, k, dev, want_keys)
        if filter is not None:
            algo = _capi.SCAN_BUCKET_TILED
        elif algo is None:
            algo = self.choose_algo(Q, P)
        stream = _stream(dev)
        while True:
            tkey, window, max_tasks = self._task_table(algo, Q, P)
            wkey, ws = self._workspace(dev, stream, algo != _capi.SCAN_QUERY_MAJOR,
                                       _capi.lib().nlsh_scan_workspace(Q, P, k, max_tasks, self.n_buckets, d))
            try:
                self._scan_launch(q, keys, nkeys, k, algo, max_tasks, out_dist, out_idx, out_keys, ncand, status, ws,
                                  _capi.PHASE_ALL, events, window, stream, filter)
            except _capi.NlshHipError:
                self._ws.pop(wkey, None)    # a call that failed part-way may have left the counters at the head non-zero
                raise
            if not check or Q == 0:
                break
            needed, overflow = status.cpu().tolist()
            if self._settle(tkey, needed, overflow, max_tasks):     # else: segment table too small, grown: repeat
                break
        self._set_last(status, algo, window, pack, tkey, max_tasks)
        return out_dist, out_idx, ncand, out_keys

    def _settle(self, tkey, needed, overflow, max_tasks):
        """What every launch path does once the host has read a launch's status words (`needed`, `overflow`): True = the results
        stand (the table is trimmed if it was far too large); False = the task table was too small and has been grown, the caller
        repeats the launch.  Raises on a broken workspace or cell contract (`_grow_task_table`)."""
        if overflow:
            self._grow_task_table(tkey, needed, overflow)
            return False
        self._trim_task_table(tkey, needed, max_tasks)
        return True

    def _trim_task_table(self, tkey, needed, max_tasks):
        """The one-shot tiled kernel launches a workgroup per table slot: a table sized for the bucket-per-task estimate and then
        run with shared windows (a fifth of the tasks) is trimmed once the batch shape's real need is known.  Called wherever the
        host learns `needed` anyway -- the checked scan, and `query()`'s own copy of the status words (the default
        `query()` path never trimmed and kept launching mostly empty workgroups)."""
        if 3 * (needed + 1024) < max_tasks:
            self._max_tasks[tkey] = int(needed * 1.25) + 1024

    def _grow_task_table(self, tkey, needed, flag=1):
        """status[1] == 1: the task table was too small; grow it, the caller repeats the call.
        status[1] == 2: the PLAN phase found the per-bucket counters at the head of the workspace non-zero on entry
        (include/nlsh_hip.h, workspace contract): the batch got no tasks; drop the workspaces and fail loudly."""
        if flag == 3:
            self._ws.clear()
            raise _capi.NlshHipError(_capi.E_INVALID, "scan_topk(tiled): the cells hold a shared window wider than one 256-row segment "
                                                      "(cells must come from nlsh_build_cells with window_rows <= 256)")
        if flag == 2:
            self._ws.clear()
            raise _capi.NlshHipError(_capi.E_WORKSPACE, "scan_topk(bucket-major): the pair counters at the head of the workspace "
                                                        "were not zero on entry (workspace contract, include/nlsh_hip.h)")
        self._max_tasks[tkey] = int(needed * 1.25) + 1024

    def _scan_fields(self, Q, d, keys, nkeys, k, algo, max_tasks, out_dist, out_idx, out_keys, ncand, status, ws, window=None):
        """The scan's share of a launch -- everything that does not change between batches of one shape -- as plain ints under the
        field names of `_capi.StepDesc`: `_scan_launch` passes them to `nlsh_scan_topk_cells_phase_filtered`, `_step_desc` fills a descriptor
        from them.  Callers that launch many batches (the kept range plans, nlsh_amd/pipeline.py) build them once per buffer set; a
        call is then one ctypes transition."""
        a, metric = _addr, self._metric_code()
        if window is None:
            window = self.choose_window(Q, keys.shape[1], algo)
        cell_of, cell_offsets, order, n_cells = self._cells_or_buckets(window if algo == _capi.SCAN_BUCKET_TILED else 0)
        return {"corpus_sorted": self.corpus_sorted.data_ptr(), "row_stride": self.row_stride, "d": d, "gid": self.gid.data_ptr(),
                "uniq_keys": self.uniq_keys.data_ptr(), "offsets": self.offsets.data_ptr(), "bucket_order": order.data_ptr(),
                "n_buckets": self.n_buckets, "cell_of": a(cell_of), "cell_offsets": a(cell_offsets), "n_cells": n_cells,
                "inv_norm": a(self.inv_norm), "Q": Q, "qkeys": keys.data_ptr(), "nkeys": nkeys.data_ptr(), "n_probes": keys.shape[1], "k": k,
                "metric": metric, "algo": algo, "seg_rows": self.seg_rows or 512, "out_dist": out_dist.data_ptr(),
                "out_idx": out_idx.data_ptr(), "out_keys": a(out_keys), "out_ncand": ncand.data_ptr(), "status": status.data_ptr(),
                "workspace": ws.data_ptr(), "workspace_bytes": ws.numel(), "max_tasks": max_tasks}

    @staticmethod
    def _step_desc(fields, encode_args, n_multi_rows, hold_done=0, streams=None):
        """The one place a `_capi.StepDesc` is filled: the scan's `fields` (`_scan_fields`), the hasher's `encode_args(...)[0]`, the
        range's multi-probe rows and -- pipeline slots only -- `hold_done` and the (front, plan, mid, tail) stream handles.  The
        descriptor holds addresses only: its owner keeps the dims array and the packed weights alive for as long as it can be launched."""
        n_layers, dims_arr, packed_ptr, act, key_mode, n_probes = encode_args
        assert n_probes == fields["n_probes"], "the encoder's probes per row are the key table's width"
        front, plan, mid, tail = streams or (None, None, None, None)
        return _capi.StepDesc(n_layers=n_layers, act=act, key_mode=key_mode, dims=ctypes.cast(dims_arr, ctypes.c_void_p), packed=packed_ptr,
                              n_multi_rows=int(n_multi_rows), hold_done=int(hold_done), front=front, plan=plan, mid=mid, tail=tail, **fields)

    def _scan_launch(self, q, keys, nkeys, k, algo, max_tasks, out_dist, out_idx, out_keys, ncand, status, ws, phases, events=None,
                     window=None, stream=None, filter=None):
        """One `nlsh_scan_topk_cells_phase_filtered` call on the current stream (`stream`: its handle, when the caller has already looked it
        up) with caller-owned buffers (any subset of the phases).  The header defines the call with float32 storage and no filter as the
        plain `nlsh_scan_topk_cells_phase`, so every index goes through it: the storage code follows the corpus pointer, the words of
        `filter` (a checked RowFilter) or NULL end the list."""
        Q, d = q.shape
        f = self._scan_fields(Q, d, keys, nkeys, k, algo, max_tasks, out_dist, out_idx, out_keys, ncand, status, ws, window)
        before = _SCAN_ARGS_BEFORE_QUERIES(f)
        if self.storage == "pq":      # the entry of its own: codebook, dsub and the code pitch where the storage code stands; row_stride = M * dsub
            before = (before[0], self._store_dim * self.pq_dsub) + tuple(before[2:])
        # an sq8 index has the call of its own: the quantiser's two arrays stand where the storage code does
        call, store = ((_capi.lib().nlsh_scan_topk_cells_phase_sq8, (self._qlo.data_ptr(), self._qstep.data_ptr())) if self.storage == "sq8"
                       else (_capi.lib().nlsh_scan_topk_cells_phase_pq, (self._codebook.data_ptr(), self.pq_dsub, self.row_stride)) if self.storage == "pq"
                       else (_capi.lib().nlsh_scan_topk_cells_phase_filtered, (_STORAGES[self.storage][1],)))
        tail = ()
        if isinstance(filter, TagFilter):       # the tagged twin of either entry: tags, masks and mode behind the filter words
            call = _capi.lib().nlsh_scan_topk_cells_phase_sq8_tagged if self.storage == "sq8" else _capi.lib().nlsh_scan_topk_cells_phase_tagged
            masks = filter.masks(Q, q.device)      # alive until the call returns: the launch is enqueued by then (stream order)
            tail = (self.tags_sorted.data_ptr() if self.tags_sorted.numel() else masks.data_ptr(), masks.data_ptr(), filter.match)
            filter = filter.row_filter
        _capi.check(call(
            before[0], *store, *before[1:], q.data_ptr(), q.stride(0) if Q else d, *_SCAN_ARGS_AFTER_QUERIES(f),
            *_event_handles(events), _stream(q.device) if stream is None else stream, phases, None if filter is None else filter.words.data_ptr(), *tail))

    def _scan_sliced(self, q, keys, nkeys, k, want_keys, check, filter=None):
        """hash_times > 64 (eval.py:148 sweeps n_samples up to 100): the key table is scanned in column slices of
        64.  A row's keys are distinct (encode_hash de-duplicates across all probes) and buckets are disjoint (F9),
        so the slices see disjoint candidates: merging their top-k lists with the (distance, id) comparator and
        adding their candidate counts is exact."""
        from .distributed import merge_topk_device
        parts, counts = [], []
        for c0 in range(0, keys.shape[1], _capi.MAX_PROBES):
            kc = keys[:, c0:c0 + _capi.MAX_PROBES].contiguous()
            nk = (nkeys - c0).clamp(0, kc.shape[1]).to(torch.int32)
            _, _, nc, k64 = self.scan_tensors(q, kc, nk, k=k, want_keys=True, check=check, filter=filter, refine_k=0)
            parts.append(k64)
            counts.append(nc)
        packed = torch.cat([torch.stack(parts), torch.stack(counts).long()[:, :, None]], dim=2)
        dist, idx, ncand = merge_topk_device(packed, k)
        keys64 = None
        if want_keys:   # the 64-bit sort keys of the merged lists: monotone(dist) << 32 | id, ~0 for padding
            bits = dist.view(torch.int32).long() & 0xFFFFFFFF
            mono = torch.where(bits >= (1 << 31), (~bits) & 0xFFFFFFFF, bits | (1 << 31))
            # padding is (-1, +inf) -- not `idx < 0`: negative ids, -1 among them, are legal row ids (a filtered `query()` takes its list
            # lengths from these keys); for ids >= 0 the two tests agree
            pad = (idx == -1) & (dist == float("inf"))
            keys64 = torch.where(pad, torch.full_like(mono, -1), (mono << 32) | (idx.long() & 0xFFFFFFFF))
        return dist, idx, ncand, keys64

    # ------------------------------------------------------------------ radius (range) queries
    @staticmethod
    def _checked_radius(radius, Q, dev):
        """`radius=` of a range call, checked before anything is launched -> float32 [Q] on `dev`."""
        if isinstance(radius, torch.Tensor):
            if radius.dtype != torch.float32:
                raise ValueError(f"radius must be a Python float or a float32 tensor, got dtype {radius.dtype}")
            if radius.dim() != 1 or radius.shape[0] != Q:
                raise ValueError(f"radius must hold one value per query: shape {tuple(radius.shape)} != ({Q},)")
            if radius.device != dev:
                raise ValueError(f"radius is on {radius.device}, the queries on {dev}")
            if Q and bool(torch.isnan(radius).any()):
                raise ValueError("radius holds a NaN: no distance compares <= NaN")
            return radius.contiguous()
        if isinstance(radius, bool) or not isinstance(radius, numbers.Real):
            raise ValueError(f"radius must be a Python float or a float32 tensor, got {type(radius).__name__}")
        if radius != radius:
            raise ValueError("radius is NaN: no distance compares <= NaN")
        with np.errstate(over="ignore"):
            r32 = np.full((Q,), radius, dtype=np.float64).astype(np.float32)    # the float32 the kernel compares with (beyond its range: +-inf)
        return torch.as_tensor(r32).to(dev)

    def _refuse_range_on_sq8(self):
        if self.storage in ("sq8", "pq"):
            raise NotImplementedError(f"radius (range) queries are not built for storage={self.storage!r}: the range kernels read float32, "
                                      "float16 and uint8 rows only (DESIGN.md 7)")

    def _range_call_checks(self, what, filter, tag_mask):
        """What every range call refuses before it does anything, in this order -> the checked filter."""
        self._refuse_tags(what, tag_mask)
        self._refuse_refine(what)
        self._refuse_range_on_sq8()
        filter = self._checked_filter(filter)
        if self.metric not in ("l2", "cosine"):
            raise NotImplementedError("range queries need metric 'l2' or 'cosine' (use SIFT.distance / Glove.distance)")
        return filter

    def _metric_code(self):
        return (_capi.METRIC_L2_EPS_FOLDED if self.l2_form == "folded" else _capi.METRIC_L2_EPS) if self.metric == "l2" else _capi.METRIC_COSINE

    def _range_head(self, q, keys, nkeys, window, filter, rad):
        """The arguments `nlsh_range_count` and `nlsh_range_fill` share, in their order: index, queries, key table, metric, schedule,
        filter words (or None) and radii."""
        a = _addr
        cell_of, cell_offsets, order, n_cells = self._cells_or_buckets(window)
        return (self.corpus_sorted.data_ptr(), _STORAGES[self.storage][1], self.row_stride, q.shape[1], self.gid.data_ptr(),
                self.uniq_keys.data_ptr(), self.offsets.data_ptr(), order.data_ptr(), self.n_buckets, a(cell_of), a(cell_offsets), n_cells,
                a(self.inv_norm), q.data_ptr(), q.stride(0), q.shape[0], keys.data_ptr(), nkeys.data_ptr(), keys.shape[1],
                self._metric_code(), _capi.SCAN_BUCKET_TILED, a(filter.words) if filter is not None else None, rad.data_ptr())

    def range_scan_tensors(self, query_vectors, keys, nkeys, radius, filter=None, limit=None, want_keys=False, tag_mask=None):
        """Radius query on a device key table -> (offsets int64 [Q + 1], idx int32 [T], dist float32 [T], ncand int32 [Q], keys64 | None),
        all on the device: query q's result is idx / dist [offsets[q]:offsets[q + 1]], EVERY row of its keys' buckets with
        dist <= radius[q] (IEEE float32: a NaN distance never is, +inf only at radius +inf), each once, in the (distance, row id) order
        of the top-k calls, with the distance bits `scan_tensors` reports for that (query, row).  DESIGN.md 4.12.
        radius: a Python float (every query's) or a float32 tensor [Q] on the queries' device.  filter: as in `scan_tensors`.
        ncand: the rows of the probed buckets, before the radius and before the filter -- `scan_tensors`' value.
        limit (None = off): ValueError once the counts are known and before any output is allocated, if T > limit.
        Two scan launches with one host read between them (`nlsh_range_count`, `nlsh_range_fill`): the call synchronises.  Always the
        tiled schedule, as filtered and compressed calls; key tables wider than 64 probes are refused."""
        filter = self._range_call_checks("range_scan_tensors", filter, tag_mask)
        q = self._as_queries(query_vectors)
        Q, d = q.shape
        if d != self.dim:
            raise ValueError(f"query dim {d} != corpus dim {self.dim}")
        P = keys.shape[1]
        if P > _capi.MAX_PROBES:
            raise ValueError(f"range queries take at most {_capi.MAX_PROBES} keys per query (hash_times <= {_capi.MAX_PROBES}), got {P}")
        if limit is not None and limit < 0:
            raise ValueError(f"limit must be None or >= 0, got {limit}")
        dev = q.device
        rad = self._checked_radius(radius, Q, dev)
        keys, nkeys = keys.contiguous(), nkeys.contiguous()
        algo, stream, L = _capi.SCAN_BUCKET_TILED, _stream(dev), _capi.lib()
        pack = torch.empty((2 * Q + 2,), dtype=torch.int32, device=dev)     # one copy brings counts, candidate counts and status to the host
        count, ncand, status = pack.split((Q, Q, 2))
        if Q == 0:
            return (torch.zeros((1,), dtype=torch.int64, device=dev), torch.empty((0,), dtype=torch.int32, device=dev),
                    torch.empty((0,), dtype=torch.float32, device=dev), ncand, torch.empty((0,), dtype=torch.int64, device=dev) if want_keys else None)
        while True:
            tkey, window, max_tasks = self._task_table(algo, Q, P)
            wkey, ws = self._workspace(dev, stream, True, L.nlsh_range_workspace(Q, P, max_tasks, self.n_buckets, d))
            head = self._range_head(q, keys, nkeys, window, filter, rad)
            tail = (status.data_ptr(), ws.data_ptr(), ws.numel(), max_tasks)
            try:
                _capi.check(L.nlsh_range_count(*head, count.data_ptr(), ncand.data_ptr(), *tail, None, None, stream))
            except _capi.NlshHipError:
                self._ws.pop(wkey, None)    # a call that failed part-way may have left the counters at the head non-zero
                raise
            host = pack.cpu()
            needed, overflow = host[2 * Q:].tolist()
            if self._settle(tkey, needed, overflow, max_tasks):     # else: task table too small, grown: count again
                break
        offsets_h = torch.zeros((Q + 1,), dtype=torch.int64)
        offsets_h[1:] = torch.cumsum(host[:Q].long(), 0)
        T = int(offsets_h[-1])
        if limit is not None and T > limit:
            raise ValueError(f"range query: {T} rows are in range, limit={limit}")
        if T >= 1 << 31:
            raise ValueError(f"range query: {T} rows are in range; one call returns fewer than 2^31 (split the batch)")
        offsets = offsets_h.to(dev)
        idx = torch.empty((T,), dtype=torch.int32, device=dev)
        dist = torch.empty((T,), dtype=torch.float32, device=dev)
        keys64 = torch.empty((T,), dtype=torch.int64, device=dev) if want_keys else None
        if T:
            sort_bytes = L.nlsh_range_sort_workspace(Q, T)
            if sort_bytes == 0:
                _capi.check(_capi.E_HIP)
            sort_ws = torch.empty((sort_bytes,), dtype=torch.uint8, device=dev)
            cursor = torch.empty((Q,), dtype=torch.int32, device=dev)
            # the fill launch runs on the plan the count call left in `ws`: same table, same workspace, nothing in between
            _capi.check(L.nlsh_range_fill(*head, offsets.data_ptr(), T, cursor.data_ptr(), _addr(keys64), dist.data_ptr(), idx.data_ptr(), *tail,
                                          sort_ws.data_ptr(), sort_bytes, None, None, stream))
        self._set_last(status, algo, window, pack, tkey, max_tasks)
        return offsets, idx, dist, ncand, keys64

    def range_tensors(self, query_vectors, radius, hash_times=10, seed=None, probes=None, candidate_budget=None, filter=None, limit=None,
                      want_keys=False, tag_mask=None):
        """Device-resident radius query: the hash by the two-step route (`last_query_path == "two_step"`; probes / candidate_budget as in
        `query_tensors`), then `range_scan_tensors`.  hash_times <= 64."""
        filter = self._range_call_checks("range_tensors", filter, tag_mask)
        if hash_times > _capi.MAX_PROBES:
            raise ValueError(f"range queries take hash_times <= {_capi.MAX_PROBES}, got {hash_times}")
        q = self._as_queries(query_vectors)
        self._checked_radius(radius, q.shape[0], q.device)      # refused before the hash is launched
        keys, nkeys = self._filtered_keys(q, hash_times, seed, probes, candidate_budget)
        return self.range_scan_tensors(q, keys, nkeys, radius, filter=filter, limit=limit, want_keys=want_keys)

    @staticmethod
    def _range_lists(offsets, idx, dist, ncand, return_distances):
        off = offsets.cpu().tolist()
        ids, nc = idx.cpu().tolist(), ncand.cpu().tolist()
        rows = [ids[lo:hi] for lo, hi in zip(off[:-1], off[1:])]
        if not return_distances:
            return rows, nc
        dh = dist.cpu().tolist()
        return rows, nc, [dh[lo:hi] for lo, hi in zip(off[:-1], off[1:])]

    def range_query(self, query_vectors, radius, hash_times=10, seed=None, probes=None, candidate_budget=None, filter=None, limit=None,
                    return_distances=False, tag_mask=None):
        """Radius query in the shape `query()` returns: (List[List[int]], List[int]) -- per query the ids of every candidate within
        `radius`, in (distance, row id) order, and the candidate counts (before the radius and the filter); with return_distances=True
        also the lists of distances.  See `range_scan_tensors`."""
        filter = self._range_call_checks("range_query", filter, tag_mask)
        out = self.range_tensors(query_vectors, radius, hash_times, seed, probes, candidate_budget, filter, limit)
        return self._range_lists(*out[:4], return_distances)

    def range_query_with_keys(self, query_vectors, key_lists: Sequence[Sequence[int]], radius, filter=None, return_distances=False,
                              tag_mask=None):
        """`range_query` on caller-supplied key lists, like `query_with_keys`."""
        filter = self._range_call_checks("range_query_with_keys", filter, tag_mask)
        _, keys, nkeys = self._pack_key_lists(key_lists, query_vectors.device)
        out = self.range_scan_tensors(query_vectors, keys, nkeys, radius, filter=filter)
        return self._range_lists(*out[:4], return_distances)

    def query_tensors(self, query_vectors, k=10, hash_times=10, seed=None, want_keys=False, check=True, events=None, probes=None,
                      candidate_budget=None, filter=None, refine_k=None, tag_mask=None, tag_match="any"):
        """Device-resident form of `query`: hashing + scan, nothing copied to the host.
        tag_mask / tag_match (an index built with `tags=` only; None = off): per-query tag filters, see `scan_tensors`.  A tagged call
        takes the route a filtered one takes: two-step, tiled schedule, counts and `candidate_budget` before the tags.
        refine_k (an index built with `refine=` only): None = stage one at k1 = min(256, max(k, refine_factor * k)), an integer in
        [k, 256] = stage one at that k1, 0 = no second stage for this call.  With the stage on, the distances are the exact float32
        ones of the ORIGINAL rows, `ncand` is stage one's, keys64 stage two's and `last_query_path` ends in "+refine".
        events = (begin, end) torch.cuda.Event pair (already recorded once) bracketing the scan kernel.
        probes ("sampled" | "ranked", None = the hasher's `probes` attribute): the multi-probe mode of this call.
        candidate_budget (ranked mode only; None = off): a query probes its ranked keys until their buckets hold that many candidates,
        `hash_times` keys at the most.
        filter (a `RowFilter` of this index; None = off): see `scan_tensors`.  A filtered call takes the two-step route (hash, then the
        filtered tiled scan; `last_query_path == "two_step"`), never the fused or the ranked one-call route.  The candidate counts and
        `candidate_budget` count bucket rows BEFORE the filter: the probe kernel does not know it."""
        filter = self._checked_filter(filter, None, tag_mask, tag_match, query_vectors)
        k1 = self._refine_k1(k, refine_k)
        if k1:
            one = self.query_tensors(query_vectors, k=k1, hash_times=hash_times, seed=seed, check=check, events=events, probes=probes,
                                     candidate_budget=candidate_budget, filter=filter, refine_k=0)
            return self._rerank(query_vectors, one, k, want_keys, check)
        if filter is not None:
            keys, nkeys = self._filtered_keys(query_vectors, hash_times, seed, probes, candidate_budget)
            return self.scan_tensors(query_vectors, keys, nkeys, k=k, want_keys=want_keys, check=check, events=events, filter=filter, refine_k=0)
        if candidate_budget is not None:
            budget = self._candidate_budget(candidate_budget, probes)
            q = self._as_queries(query_vectors)
            algo = self.choose_algo(q.shape[0], hash_times)
            if self._fuses_ranked(q, hash_times, algo, ranked=True):
                return self._ranked_tensors(q, k, hash_times, budget, want_keys, check, events, algo, self._n_multi_rows(q.shape[0]))[:4]
            self.last_query_path = "two_step"
            keys, nkeys, _ = self._hash_budget(q, HASH_BATCH, hash_times, budget)
            return self.scan_tensors(q, keys, nkeys, k=k, want_keys=want_keys, check=check, events=events, refine_k=0)
        if probes is None:
            return self._batch_tensors(query_vectors, k, hash_times, seed, want_keys=want_keys, check=check, events=events)[:4]
        with self._probe_mode(probes):
            return self._batch_tensors(query_vectors, k, hash_times, seed, want_keys=want_keys, check=check, events=events)[:4]

    def _filtered_keys(self, query_vectors, hash_times, seed, probes, candidate_budget):
        """The key table of a filtered call: always the two-step route's first step, whatever the probe mode."""
        if hash_times < 1:
            raise ValueError(f"`n` should be positive integer, but got {hash_times}")
        self.last_query_path = "two_step"
        q = self._as_queries(query_vectors)
        if candidate_budget is not None:
            return self._hash_budget(q, HASH_BATCH, hash_times, self._candidate_budget(candidate_budget, probes))[:2]
        return self.hash_device(q, hash_times=hash_times, seed=seed, probes=probes)

    def _filtered_lists(self, idx, ncand, keys64):
        """Device results of a filtered call -> (lists, candidate counts).  A list's length comes from its sort keys (~0 = padding), not
        from `idx >= 0`: -1 is a legal row id."""
        idx_h, nc_h = idx.cpu().numpy(), ncand.cpu().numpy()
        lens = (keys64 != -1).sum(dim=1).cpu().numpy()
        rows, counts = self._plain_lists(np.ascontiguousarray(idx_h), nc_h)
        k = idx_h.shape[1] if idx_h.ndim == 2 else 0
        for qi in np.nonzero(lens < k)[0].tolist():
            rows[qi] = rows[qi][:int(lens[qi])]
        return rows, counts

    def _fuses(self, q, hash_times, algo):
        """One `nlsh_query_batch` call (ABI v4: five launches, the bucket lookup in the encode's epilogue) serves a batch when the
        fused kernel may hash it at all (not a BatchNorm encoder in train mode), the key table fits one scan call and the schedule
        is a bucket-major one (the query-major stream's PLAN phase is a single kernel of its own).  A streamed encoder (hidden layer
        wider than `_capi.MAX_WIDTH`) has no fused encode launch: `hash_device` + `scan_tensors`, the same results by design.  Neither
        has a ranked hasher (`probes="ranked"`): its keys come from `nlsh_probe_ranked` behind the encode."""
        return self._one_call_form(q, hash_times, algo, "encode_args") and getattr(self._hashing, "probes", "sampled") != "ranked"

    def _one_call_form(self, q, hash_times, algo, encode_args):
        """What `_fuses` and `_fuses_ranked` both need (`encode_args`: the hasher method that fills the form's descriptor).  The storage
        test comes first: on a compressed index nothing else is looked at, the batch included."""
        if self.compressed:         # the step descriptor has no storage field: a compressed index hashes, then calls the typed scan
            return False
        h = self._hashing
        needs_train = getattr(h, "_needs_train_forward", None)
        streamed = getattr(h, "streamed", None)
        return (self.metric in ("l2", "cosine") and 1 <= hash_times <= _capi.MAX_PROBES and algo != _capi.SCAN_QUERY_MAJOR
                and self.n_buckets > 0 and q.shape[0] > 0 and not (needs_train is not None and needs_train())
                and hasattr(h, encode_args) and not (streamed is not None and streamed()))

    # The ranked mode's one-call form (`nlsh_query_batch_ranked`: five launches, the keys looked up by the kernel that ranks them) against
    # its two-step form (`hash_device` / `_hash_budget` + `scan_tensors`: seven launches); same results, bit for bit.  OFF by default: on
    # the SIFT1M-shaped batch the one-call form measured slower than the two-step form in five of six comparisons (device-resident
    # batch: +0.030 / +0.015 / +0.051 ms at hash_times 10 / 32 / budget 3000; `query()`: -0.030 / +0.061 / +0.032 ms;
    # profiles/ranked_one_call.txt, tools/ranked_path_bench.py) -- the fused kernel takes longer than the two it replaces and the
    # launches it saves were not idle time.  True selects it (the tests and the A/B tool do); DESIGN.md 4.7 has the analysis.
    ranked_one_call = False
    # which form served the last `query_tensors` / `query` call: "fused" (sampled, `nlsh_query_batch`) | "ranked_one_call" | "two_step",
    # with "+refine" behind it when the exact re-rank ran behind that form (an index built with refine=)
    last_query_path = None

    def _fuses_ranked(self, q, hash_times, algo, ranked=None):
        """One `nlsh_query_batch_ranked` call serves a ranked batch (`ranked`: the call said so -- a candidate budget implies the mode --;
        None = the hasher's `probes` attribute, which a call's `probes=` sets for its duration), with or without a budget, under the
        conditions of `_fuses`: a device metric, a key table of one scan call, a bucket-major schedule on a non-empty index, a non-empty
        batch, an LDS-resident encoder and no BatchNorm train-mode forward.  Everything else keeps the two-step path."""
        if self.compressed or not self.ranked_one_call:
            return False
        if ranked is None:
            ranked = getattr(self._hashing, "probes", "sampled") == "ranked"
        return bool(ranked) and self._one_call_form(q, hash_times, algo, "ranked_encode_args")

    def _ranked_scratch(self, m, dev):
        """Fresh scratch of one `nlsh_query_batch_ranked` call of m rows (z, hard codes, the one-probe encode's own key table)."""
        need = _capi.lib().nlsh_query_batch_ranked_scratch(m, self._hashing.output_dim)
        if need == 0:
            _capi.check(_capi.E_UNSUPPORTED)
        return torch.empty((need,), dtype=torch.uint8, device=dev)

    def _one_call(self, q, k, P, want_keys, check, algo, n_multi, out, start):
        """The launch loop of the two one-call forms (`_batch_tensors` where `_fuses` holds, `_ranked_tensors`): fresh outputs, the key
        table `out` or a fresh one, then the call -- repeated on the keys the first one left, scan part only (`lookup_done`), while the
        task table overflows -> (dist, idx, ncand, keys64 | None, keys, nkeys).  `start(keys, nkeys)`, called once behind the dim check
        and the allocations, gives what is the form's own: the hasher's encode arguments for the descriptor and
        call(desc, lookup_done, stream), which makes the C call and returns its status."""
        Q, d = q.shape
        if d != self.dim:
            raise ValueError(f"query dim {d} != corpus dim {self.dim}")
        L, dev = _capi.lib(), q.device
        if out is not None:
            keys, nkeys = out
        else:
            keys = torch.empty((Q, P), dtype=torch.int32, device=dev)
            nkeys = torch.empty((Q,), dtype=torch.int32, device=dev)
        out_dist, pack, out_idx, ncand, status, out_keys = self._outputs(Q, k, dev, want_keys)
        enc, call = start(keys, nkeys)              # (`enc` held to the end of the call: the descriptor names its dims array)
        stream = _stream(dev)
        lookup_done = 0
        while True:
            tkey, window, max_tasks = self._task_table(algo, Q, P)
            wkey, ws = self._workspace(dev, stream, True, L.nlsh_scan_workspace(Q, P, k, max_tasks, self.n_buckets, d))
            desc = self._step_desc(self._scan_fields(Q, d, keys, nkeys, k, algo, max_tasks, out_dist, out_idx, out_keys, ncand, status, ws,
                                                     window), enc, n_multi)
            try:
                _capi.check(call(desc, lookup_done, stream))
            except _capi.NlshHipError:
                self._ws.pop(wkey, None)    # a call that failed part-way may have left the counters at the head non-zero
                raise
            if not check:
                break
            needed, overflow = status.cpu().tolist()
            if self._settle(tkey, needed, overflow, max_tasks):
                break
            lookup_done = 1                 # task table too small, grown: repeat the scan part on the same keys
        self._set_last(status, algo, window, pack, tkey, max_tasks)
        return out_dist, out_idx, ncand, out_keys, keys, nkeys

    def _ranked_tensors(self, q, k, P, budget, want_keys, check, events, algo, n_multi, out=None):
        """`_batch_tensors` of the ranked mode where `_fuses_ranked` holds: one `nlsh_query_batch_ranked` call with fresh outputs
        (`budget` None = no budget)."""
        def start(keys, nkeys):
            enc = self._hashing.ranked_encode_args(P)
            scratch = self._ranked_scratch(q.shape[0], q.device)
            return enc, lambda desc, lookup_done, stream: _capi.lib().nlsh_query_batch_ranked(
                ctypes.byref(desc), ctypes.sizeof(desc), q.data_ptr(), q.stride(0), lookup_done, budget or 0, scratch.data_ptr(), scratch.numel(),
                None, 0, *_event_handles(events), stream)
        got = self._one_call(q, k, P, want_keys, check, algo, n_multi, out, start)
        self.last_query_path = "ranked_one_call"
        return got

    def _batch_tensors(self, query_vectors, k, hash_times, seed, want_keys=False, check=True, events=None, algo=None, row0=0,
                       n_multi=None, out=None):
        """hash + scan of one batch (or one row range of a batch: `row0`, `n_multi` = rows of the RANGE that are multi-probe, `out` =
        the range's slice of the batch's key table) -> (dist, idx, ncand, keys64 | None, keys, nkeys).  One C-ABI call where the
        fused form applies (`_fuses`), `hash_device` + `scan_tensors` otherwise; same results either way, bit for bit."""
        if hash_times < 1:
            raise ValueError(f"`n` should be positive integer, but got {hash_times}")
        q = self._as_queries(query_vectors)
        Q = q.shape[0]
        if algo is None:
            algo = self.choose_algo(Q, hash_times)
        if n_multi is None:
            n_multi = self._n_multi_rows(Q)
        if self._fuses_ranked(q, hash_times, algo):
            return self._ranked_tensors(q, k, hash_times, None, want_keys, check, events, algo, n_multi, out)
        fuses = self._fuses(q, hash_times, algo)
        self.last_query_path = "fused" if fuses else "two_step"
        if not fuses:
            if row0 or out is not None:
                keys, nkeys = self._hashing.hash_device(q, n=hash_times, n_multi_rows=n_multi, seed=seed, row0=row0, out=out)
            else:
                keys, nkeys = self.hash_device(q, hash_times=hash_times, seed=seed)
            return self.scan_tensors(q, keys, nkeys, k=k, want_keys=want_keys, check=check, events=events, algo=algo, refine_k=0) + (keys, nkeys)

        def start(keys, nkeys):     # the seed is drawn behind the dim check: a call refused there takes none
            s = self._hashing.next_seed() if seed is None else seed
            return self._hashing.encode_args(hash_times, keys, nkeys)[0], lambda desc, lookup_done, stream: _capi.lib().nlsh_query_batch(
                ctypes.byref(desc), ctypes.sizeof(desc), q.data_ptr(), q.stride(0), s, int(row0), lookup_done, *_event_handles(events), stream)
        return self._one_call(q, k, hash_times, want_keys, check, algo, n_multi, out, start)

    def _rows_of_key(self, key):
        """Ascending global row ids of one bucket (host list) or [] for an unknown key.  Called once per query with fewer than k
        candidates (the reference's F7 rule) -- ~20 times per 10^4-query batch on the headline workload, so it is a dict lookup and a
        slice of host copies made once per index, not numpy searches (those cost 4 us per call: 0.07 ms of a 0.88-ms `query()`)."""
        key = int(key)
        if self._hashing.key_mode == _capi.KEY_FULL and key >= (1 << 31):
            key -= 1 << 32
        directory = self.__dict__.get("_bucket_dir")
        if directory is None:   # signed int32 key -> (first sorted row, end): one pass over the CSR, once per index
            directory = self._bucket_dir = dict(zip(self._uniq_host.tolist(), zip(self._offs_host[:-1].tolist(), self._offs_host[1:].tolist())))
        span = directory.get(key)
        if span is None:
            return []
        if self._perm_host is None:   # one D2H of the permutation, then every fallback list is a host slice
            self._perm_host = self.gid.cpu().numpy().astype(np.int64)
        return self._perm_host[span[0]:span[1]].tolist()

    # `query()` launches the same row ranges of the same batch shape call after call, and everything it needs on the device is consumed
    # before it returns (the results leave as Python lists).  So the range's buffers -- its slice of the batch's key table, distances,
    # the id / count / status block -- and the descriptor of its `nlsh_query_batch` call are built ONCE per (batch shape, range, k,
    # schedule) and kept: a later call checks that the task table, the workspace and the hasher's weights are still the ones the
    # descriptor names and makes its one C call.  r06: the Python around that call (allocations, the descriptor's forty fields, the
    # weight walk, argument tuples) was 0.08 ms per range = 0.2 ms of a 1.1-ms call (tools/query_host_profile.py).  `query_tensors`
    # hands its tensors to the caller and keeps allocating fresh ones.  Like the scan workspace (one per stream), the kept buffers
    # assume one `query()` at a time per indexer and stream.
    def _range_plan(self, q, keys, nkeys, k, lo, hi, algo, n_multi, host=None, ranked=False):
        """`ranked`: the plan of an `nlsh_query_batch_ranked` call -- the hasher's `ranked_encode_args` in the descriptor and the call's
        scratch kept beside the other buffers."""
        Q_all, P = keys.shape
        dev, m = q.device, hi - lo
        stream = _stream(dev)
        ckey = (stream, Q_all, lo, hi, P, k, algo, self.l2_form, keys.data_ptr(), q.shape[1], ranked)
        plans = self.__dict__.setdefault("_range_plans", {})
        plan = plans.get(ckey)
        tkey, window, max_tasks = self._task_table(algo, m, P)
        sig = self._hashing._weights_signature()
        # `host`: the range's slice of the pinned result block (`_host_form`); the plan keeps its address and size only (a reference would
        # hold an outgrown block's pinned pages for as long as the plan lives) -- the block is reallocated when a larger batch shape
        # arrives, and a plan that names another address than the call's slice is rebuilt before it is used
        host_ptr = None if host is None else host.data_ptr()
        if (plan is not None and plan["max_tasks"] == max_tasks and plan["ws"] is self._ws.get(plan["wkey"]) and plan["window"] == window
                and plan["host_ptr"] == host_ptr):
            if plan["sig"] != sig:        # a training step between two calls: the descriptor gets the new blob
                plan["packed"] = self._hashing.packed_weights()
                plan["desc"].packed = plan["packed"].data_ptr()
                plan["sig"] = sig
            return plan
        d = q.shape[1]
        wkey, ws = self._workspace(dev, stream, True, _capi.lib().nlsh_scan_workspace(m, P, k, max_tasks, self.n_buckets, d))
        rk, rn = keys[lo:hi], nkeys[lo:hi]
        out_dist, pack, out_idx, ncand, status, _ = self._outputs(m, k, dev)
        enc = self._hashing.ranked_encode_args(P) if ranked else self._hashing.encode_args(P, rk, rn)[0]
        scratch = self._ranked_scratch(m, dev) if ranked else None
        desc = self._step_desc(self._scan_fields(m, d, rk, rn, k, algo, max_tasks, out_dist, out_idx, None, ncand, status, ws, window),
                               enc, min(max(n_multi - lo, 0), m))
        plan = plans[ckey] = dict(desc=desc, ref=ctypes.byref(desc), size=ctypes.sizeof(desc), dims_arr=enc[1], packed=self._hashing.packed_weights(), sig=sig,
                                  keys=rk, nkeys=rn, out_dist=out_dist, pack=pack, status=status, ws=ws, wkey=wkey, max_tasks=max_tasks, tkey=tkey,
                                  window=window, stream=stream, host_ptr=host_ptr, host_words=0 if host is None else host.numel(),
                                  scratch=scratch, scratch_ptr=None if scratch is None else scratch.data_ptr(),
                                  scratch_bytes=0 if scratch is None else scratch.numel())
        if len(plans) > 64:           # batch shapes come and go (a caller sweeping Q): keep the dictionary bounded
            for old_key in list(plans)[:-32]:
                del plans[old_key]
        return plan

    def _host_form(self, k, fused):
        """Whether a row range's results reach the host from the merge kernel itself (`nlsh_query_batch_host`: no copy command behind the
        kernels) -- the fused call with k <= 64.  Everything else (a streamed encoder, the query-major schedule, hash_times > 64: not
        `fused`; wide k) keeps the device->host copies."""
        return fused is not None and k <= _capi.MAX_K

    def _range_tensors(self, q, keys, nkeys, k, lo, hi, algo, fused, host=None):
        """One row range of a `query()` batch on the stream: `fused` = (hash_times, seed, rows of the batch that are multi-probe) --
        the range is hashed AND scanned by one `nlsh_query_batch` call into its slice of the batch's key table; ("ranked", budget or 0,
        multi-probe rows): the same with one `nlsh_query_batch_ranked` call (no seed, no row offset: ranked keys are a function of the
        row alone); None: the table was filled by a whole-batch `hash_device` and the range is only scanned.  `host` (`_host_form`): the range's slice of the pinned
        result block -- the call is `nlsh_query_batch_host`, whose merge kernel stores ids | counts | status | the short queries' key rows
        there, and nothing has to be copied afterwards."""
        if fused is None:
            if hi - lo == q.shape[0]:     # the whole batch (`_host_results`): nothing to slice
                self.scan_tensors(q, keys, nkeys, k=k, check=False, algo=algo, refine_k=0)
            else:
                self.scan_tensors(q[lo:hi], keys[lo:hi], nkeys[lo:hi], k=k, check=False, algo=algo, refine_k=0)
            return
        mode, seed, n_multi = fused
        ranked = mode == "ranked"
        plan = self._range_plan(q, keys, nkeys, k, lo, hi, algo, n_multi, host, ranked)
        qr = q[lo:hi]
        try:
            if ranked:          # `seed` holds the budget (0 = none); host_ptr None = the results stay on the device (wide k)
                _capi.check(_capi.lib().nlsh_query_batch_ranked(plan["ref"], plan["size"], qr.data_ptr(), qr.stride(0), 0, seed, plan["scratch_ptr"],
                                                                plan["scratch_bytes"], plan["host_ptr"], plan["host_words"], None, None, plan["stream"]))
            elif host is not None:
                _capi.check(_capi.lib().nlsh_query_batch_host(plan["ref"], plan["size"], qr.data_ptr(), qr.stride(0), seed, lo, 0, plan["host_ptr"],
                                                              plan["host_words"], plan["stream"]))
            else:
                _capi.check(_capi.lib().nlsh_query_batch(plan["ref"], plan["size"], qr.data_ptr(), qr.stride(0), seed, lo, 0, None, None, plan["stream"]))
        except _capi.NlshHipError:
            self._ws.pop(plan["wkey"], None)    # a call that failed part-way may have left the counters at the head non-zero
            self._range_plans.clear()
            raise
        self._set_last(plan["status"], algo, plan["window"], plan["pack"], plan["tkey"], plan["max_tasks"])

    @staticmethod
    def _block_views(a, m, k, P, host_form):
        """A range's block of the pinned buffer (host array of m*k + m + 2 + m*P + m words) -> (ids [m, k], counts [m], keys [m, P],
        nkeys [m]).  Behind the ids | counts | status words the copy form holds keys | nkeys; the host-writing merge stores key rows
        [m, P + 1] there -- nkeys, then the keys -- written for the queries with < k candidates only."""
        n = m * k + m + 2
        ids, counts = a[:m * k].reshape(m, k), a[m * k:m * k + m]
        if host_form:
            rows = a[n:n + m * (P + 1)].reshape(m, P + 1)
            return ids, counts, rows[:, 1:], rows[:, 0]
        return ids, counts, a[n:n + m * P].reshape(m, P), a[n + m * P:n + m * P + m]

    def _range_copied(self, q, keys, nkeys, k, lo, hi, algo, fused, block):
        """The copy form of one row range: `_range_tensors` with the results left on the device, then device->host copies on the stream
        into the head of the range's `block` of the pinned buffer -- ids | counts | status, and under `compat` the key table and its
        counts.  A range that is the whole batch slices nothing: every tensor view made here is host time of the call."""
        m, P = hi - lo, keys.shape[1]
        self._range_tensors(q, keys, nkeys, k, lo, hi, algo, fused)
        n = m * k + m + 2
        to_ids, to_keys, to_nkeys, _ = block.split((n, m * P, m, block.numel() - n - m * P - m))
        to_ids.copy_(self._last_pack, non_blocking=True)
        if self.compat:
            whole = m == keys.shape[0]
            to_keys.view(m, P).copy_(keys if whole else keys[lo:hi], non_blocking=True)
            to_nkeys.copy_(nkeys if whole else nkeys[lo:hi], non_blocking=True)

    def _host_results(self, q, keys, nkeys, k, fused=None, queued=None):
        """One range = the whole batch: scan, results into the pinned block, ONE stream synchronisation (the only sync of a `query()`
        call).  `queued`: called once, between the launch and that synchronisation (`_Shells.alloc`: host work that needs no result).
        `_host_form`: the merge kernel stores ids | counts | status | the short queries' key rows there itself and nothing is
        copied.  Otherwise: device->host copies of (ids, candidate counts, status) and of the key table (it rides along because the F7
        rule needs the key sets of the few queries with < k candidates: 400 KB more on the wire is cheaper than a second round of
        device indexing + copies + syncs after the first).  Repeats the scan if the task table overflowed."""
        Q, P = keys.shape
        algo = self.choose_algo(Q, P)
        n, words = Q * k + Q + 2, Q * k + Q + 2 + Q * P + Q
        host_form = self._host_form(k, fused) and Q > 0
        while True:
            pin = self._pin
            if pin is None or pin.numel() < words:
                pin = self._pin = torch.empty((max(words, 1 << 16),), dtype=torch.int32, pin_memory=True)
            if host_form:           # the merge kernel stores into the pinned block itself: nothing to copy
                self._range_tensors(q, keys, nkeys, k, 0, Q, algo, fused, pin[:words])
            else:
                self._range_copied(q, keys, nkeys, k, 0, Q, algo, fused, pin)
            self._release_held()                                    # the device is busy now: free what an earlier call left with us
            if queued is not None:
                queued()
                queued = None                                       # a repeated scan (task table grown) keeps what the first built
            torch.cuda.current_stream(q.device).synchronize()
            host = pin.numpy()
            if self._settle(self._last_tkey, int(host[n - 2]), int(host[n - 1]) if Q else 0, self._last_max_tasks):
                return self._block_views(host, Q, k, P, host_form)

    # `query()` on a large batch scans it in `query_chunks` row ranges on the stream and converts range c to Python lists while
    # the device scans range c+1: the conversion (0.45 ms per 10^4 queries) is as long as the scan, and a single range leaves
    # the host idle during the scan and the device idle during the conversion.  Results do not depend on the split (the hash
    # runs once over the whole batch; every query's candidates and top-k are its own; the schedule is the whole batch's).
    # None = automatic: 2 ranges, or 1 when `defer_result_release` is on -- the previous call's lists are then freed under the scan,
    # the host is the longer side of the call whatever the split, and a second range only adds its launches (r03, 10^4 queries:
    # 10.4 M queries/s with one range, 9.4 M with two, 7.6 M with three; with the release in the caller's loop 5.6 / 5.9 / 6.4 M).
    query_chunks = None
    _CHUNK_MIN_ROWS = 2048

    def _n_chunks(self):
        if self.query_chunks is not None:
            return int(self.query_chunks)
        return 1 if self.defer_result_release else 2

    def _chunked_results(self, q, keys, nkeys, k, n_chunks, fused=None, queued=None):
        """Generator over row ranges of the batch: (lo, hi, ids [hi-lo, k], counts [hi-lo], keys, nkeys) as host arrays, each
        yielded as soon as ITS scan and copies are done (one event per range; later ranges keep the device busy meanwhile).
        `queued`: called once every range is on the stream, before the first wait (`_Shells.alloc`: host work that needs no result)."""
        Q, P = keys.shape
        algo = self.choose_algo(Q, P)
        stream = torch.cuda.current_stream(q.device)
        bounds = [(Q * c // n_chunks, Q * (c + 1) // n_chunks) for c in range(n_chunks)]
        per = max(hi - lo for lo, hi in bounds)
        words = (per * k + per + 2 + per * P + per + 3) // 4 * 4     # every range's block starts on a 16-byte boundary (the host-writing merge stores 16 bytes per lane there)
        if self._pin is None or self._pin.numel() < n_chunks * words:
            self._pin = torch.empty((max(n_chunks * words, 1 << 16),), dtype=torch.int32, pin_memory=True)
        pin = self._pin
        host_form = self._host_form(k, fused)

        def launch(c, lo, hi):
            m = hi - lo
            n = m * k + m + 2
            block = pin[c * words:c * words + n + m * P + m]
            if host_form and m:     # the merge kernel stores into the range's slice of the pinned block itself: nothing to copy
                self._range_tensors(q, keys, nkeys, k, lo, hi, algo, fused, block)
            else:
                self._range_copied(q, keys, nkeys, k, lo, hi, algo, fused, block)
            ev = torch.cuda.Event()
            ev.record(stream)
            return ev, self._last_tkey, self._last_max_tasks

        inflight = [launch(c, lo, hi) for c, (lo, hi) in enumerate(bounds)]
        self._release_held()                                        # the device is busy now: free what an earlier call left with us
        if queued is not None:
            queued()
        host = pin.numpy()
        for c, (lo, hi) in enumerate(bounds):
            m = hi - lo
            a = host[c * words:(c + 1) * words]
            n = m * k + m + 2
            while True:
                ev, tkey, max_tasks = inflight[c]
                ev.synchronize()
                if self._settle(tkey, int(a[n - 2]), int(a[n - 1]) if m else 0, max_tasks):
                    break
                inflight[c] = launch(c, lo, hi)                     # task table too small for this range, grown: repeat it
            yield (lo, hi) + self._block_views(a, m, k, P, host_form and m > 0)

    # The fresh result lists (10^4 per batch) land in the collector's youngest generation; the first container allocation after
    # the conversion then runs a generation-0 collection that walks all of them: 0.25-0.32 ms of a 1.55 ms call on the bench box
    # (tools/query_host_profile.py, QGC=1).  Instead: (1) a generation-0 collection BEFORE the conversion, while the young
    # generation holds only what the application made since the last call (microseconds; its cyclic garbage is reclaimed
    # here, as it would have been); (2) the conversion with the collector paused; (3) gc.freeze() + gc.unfreeze(), which moves
    # every tracked object to the oldest generation in O(1) and zeroes the young counters, so the results are first walked by
    # the next FULL collection, like any long-lived object.  Because the counters restart from zero at every call, a tight
    # query loop would never reach the collector's thresholds for the older generations on its own: every
    # `_FULL_COLLECT_EVERY`-th promotion is followed by an explicit full collection (tens of ms in a torch process, so rare).
    # It rewrites the host application's collector generations, so it is OPT-IN (`Indexer.promote_results = True`; bench.py never
    # turns it on): by default the conversion only pauses the collector for its own duration.  Even when on it is skipped when the application holds
    # frozen objects of its own (gc.get_freeze_count() > 0) or has the collector disabled.
    promote_results = False
    # A caller that loops `ids, counts = indexer.query(batch)` frees the previous call's 10^4 lists when it rebinds the names: ~0.3 ms
    # of host time per 10^4 queries that sits between two calls, while the device idles.  OPT-IN (`Indexer.defer_result_release = True`):
    # the indexer keeps a reference to its last TWO results and drops the older one right after the NEXT call has queued its device
    # work -- the deallocation then runs under the scan instead of in front of it.  Results are unchanged and stay the caller's to keep;
    # the cost is that up to two extra result sets (a few MB of Python objects each) stay alive per indexer.  Off by default for the
    # same reason as `promote_results`: a library call should not change object lifetimes unasked.  bench.py's headline `value` is
    # measured with all of these off (r04); `protocol_qps_opt_in` is the same region with this switch and `untracked_results` on.
    defer_result_release = False
    # OPT-IN: hand the inner result lists out untracked by the cyclic collector (csrc/fastlists.c).  A row of ints cannot be part of a
    # cycle and 10^4 tracked young lists per call make the collector's next young pass cost ~0.26 ms -- but CPython never untracks
    # lists, and a caller that later stores something that references the row INTO the row would leak that cycle.  Off by default
    # like the two switches above (r03 untracked whenever the helper was built).
    untracked_results = False
    _FULL_COLLECT_EVERY = 2048
    _promotions = 0

    @classmethod
    def _plain_lists(cls, idx_h, nc_h):
        """Host arrays -> (list of id rows, list of counts): one C-level conversion each for the whole batch."""
        # the state the APPLICATION left the collector in -- not `gc.isenabled()`, which is False whenever `query()` holds its pause
        promote = _collector_pause.application_state() and cls.promote_results and len(nc_h) >= 512 and gc.get_freeze_count() == 0
        if promote:
            gc.collect(0)
        with _collector_pause:   # 10^4 fresh lists would trigger a dozen collections over the whole heap: a third of the conversion
            if _rows_to_lists is not None and idx_h.dtype == np.int32 and idx_h.ndim == 2 and idx_h.flags.c_contiguous:
                out = _rows_to_lists(idx_h, idx_h.shape[0], idx_h.shape[1], bool(cls.untracked_results)), nc_h.tolist()
            else:
                out = idx_h.tolist(), nc_h.tolist()
            if promote:
                gc.freeze()
                gc.unfreeze()
                Indexer._promotions += 1
                if Indexer._promotions % cls._FULL_COLLECT_EVERY == 0:
                    gc.collect()
            return out

    def _to_lists(self, key_sets, idx_h, nc_h, k):
        """Host arrays -> the reference's (List[List[int]], List[int]) (indexer.py:88-95)."""
        results, counts = self._plain_lists(idx_h, nc_h)
        self._replace_short(results, 0, key_sets, idx_h, nc_h, k)
        return results, counts

    def _replace_short(self, results, base, key_sets, idx_h, nc_h, k):
        """The short-query rule on rows [base, base + len(nc_h)) of `results`, whose host arrays are `idx_h` / `nc_h`."""
        for qi in np.nonzero(nc_h < k)[0].tolist():   # only the short queries need the reference's special case
            if self.compat:
                # indexer.py:89-93 (F7): topk raises -> rows of the LAST key of the set iteration
                order = list(key_sets[qi])
                results[base + qi] = self._rows_of_key(order[-1]) if order else []
            else:
                results[base + qi] = [int(v) for v in idx_h[qi] if v >= 0]

    # The containers of a result -- the outer list, its Q inner lists, the list of counts -- depend on (Q, k) only, not on a single id,
    # and building them is a fifth of the conversion (0.10 of 0.49 ms per 10^4 queries).  `query()` therefore builds them in the window in which the host would otherwise
    # sleep: after every row range is on the stream and the previous call's lists are released, before the first wait
    # (`_Shells.alloc`, the `queued` hook of `_chunked_results` / `_host_results`).  Each range's ids and counts are then stored into
    # its rows when its event completes (`_Shells.fill`), which also replaces `results += r`, `counts += c` and `nc_h.tolist()`.
    # Until a row is filled its slots are empty, so csrc/fastlists.c keeps the unfilled lists (and the outer list around them) off the
    # collector: nothing but this call's frame refers to them, and a call that raises between the phases drops them like any list.
    # The lists a caller receives are what `_plain_lists` builds, object for object: tracked unless `untracked_results`.
    # The one-shot path stays for a helper that is not built, for `promote_results`, whose generation-0 collection and freeze
    # bracket one conversion (`_plain_lists`), and for `defer_result_release`: there the previous result is released in the same
    # window (0.3 ms, longer than the scan), the host never waits, and shells built on top of that only lengthen the call (measured:
    # `protocol_qps_opt_in` 10.7 -> 9.6 M queries/s).  Every range's id block is a C-contiguous slice of the int32 pinned block, which is what
    # the helper takes (it refuses anything else).
    class _Shells:
        __slots__ = ("Q", "k", "rows", "counts")

        def __init__(self, Q, k):
            self.Q, self.k, self.rows, self.counts = Q, k, None, None

        def alloc(self):
            with _collector_pause:
                self.rows, self.counts = _rows_alloc(self.Q, self.k), [0] * self.Q

        def fill(self, lo, hi, idx_h, nc_h, untrack):
            with _collector_pause:
                _rows_fill(self.rows, lo, hi, idx_h, nc_h, self.counts, untrack)

    def _shells(self, Q, k):
        """The two-phase construction for a batch of Q queries, or None where the one-shot conversion runs (see above)."""
        if _rows_alloc is None or _rows_fill is None or self.promote_results or self.defer_result_release or Q == 0:
            return None
        return self._Shells(Q, k)

    def _fill_range(self, shells, lo, hi, idx_h, nc_h, keys_h, nkeys_h, k):
        shells.fill(lo, hi, idx_h, nc_h, bool(self.untracked_results))
        self._replace_short(shells.rows, lo, self._short_key_sets(nc_h, keys_h, nkeys_h, k), idx_h, nc_h, k)

    def _release_held(self):
        """Drop all but the newest result kept by `defer_result_release` (called once the current call's device work is queued)."""
        held = self.__dict__.get("_held")
        if held:
            del held[:-1]

    def _keep(self, result):
        if self.defer_result_release:
            held = self.__dict__.setdefault("_held", [])
            held.append(result)
            # never more than the newest two, whichever path produced them: the generic-metric and sliced (hash_times > 64) paths do
            # not pass through `_release_held`, and without this the list grew by one full result set per call
            del held[:-2]
        elif self.__dict__.get("_held"):
            self._held = []
        return result

    # The cyclic collector is paused for the length of a `query()` call, not only while a row range is converted: with tracked rows
    # (the default) every resume between two ranges is followed by a young-generation pass over the lists made so far, and every tenth
    # young pass by an older-generation one over all the tracked lists alive -- the collector's work per call grew with the number of row
    # ranges (r04, tools/query_modes.py, same box: 1 range 1.47 ms per call, 2 ranges 1.93, 4 ranges 2.66), which is what kept the split
    # from paying.  Paused across the call the fresh lists are walked once, after the call, whatever the split.  No generation is
    # rewritten and nothing is frozen (unlike `promote_results`): the collector simply does not run inside the call, as it already did
    # not inside the conversions.  False restores r04's behaviour (tools/query_modes.py times both).
    # The pause is `_collector_pause`: one re-entrant, lock-protected region counter for the whole process, so concurrent `query()` calls
    # of two threads and the nested pause of `_plain_lists` leave the collector as the FIRST of them found it (r06).
    pause_collector_for_call = True

    def _query_two_step(self, query_vectors, k, k1, hash_times, seed, probes, candidate_budget, filter):
        """`query()` of a filtered call (k1 = 0) and of an index with refine= (k1: stage one's k): the two-step route's key table, the
        scan -- with the re-rank behind it, `last_query_path == "two_step+refine"` -- and one copy to the host.  Unfiltered, the
        short-query rule (F7) is applied from stage one's candidate counts, as on an unrefined index."""
        keys, nkeys = self._filtered_keys(query_vectors, hash_times, seed, probes, candidate_budget)
        _, idx, ncand, keys64 = self.scan_tensors(query_vectors, keys, nkeys, k=k, want_keys=True, filter=filter, refine_k=k1)
        if filter is not None:
            return self._filtered_lists(idx, ncand, keys64)
        idx_h, nc_h = np.ascontiguousarray(idx.cpu().numpy()), ncand.cpu().numpy()
        keys_h, nkeys_h = (keys.cpu().numpy(), nkeys.cpu().numpy()) if self.compat else (None, None)
        return self._to_lists(self._short_key_sets(nc_h, keys_h, nkeys_h, k), idx_h, nc_h, k)

    def query(self, query_vectors, k=10, hash_times=10, seed=None, probes=None, candidate_budget=None,
              filter=None, refine_k=None, tag_mask=None, tag_match="any") -> Tuple[List[List[int]], List[int]]:
        """nlsh/indexer.py:56-96.  `seed` (not in the reference): the Philox seed of the multi-probe draws; None takes the next one
        from the hasher's call counter, like every other hashing call.  `probes` (not in the reference): "sampled" | "ranked", the
        multi-probe mode of this call; None = the hasher's `probes` attribute.  `candidate_budget` (not in the reference; ranked mode
        only, None = off): a query probes its ranked keys until their buckets hold that many candidates, `hash_times` keys at the most.
        `filter` (not in the reference; a `RowFilter` of this index, `row_filter()`; None = off): every list holds allowed ids only, in
        (distance, id) order, min(k, allowed candidates) of them -- what the index over the allowed rows alone returns with
        compat=False.  The reference's "fewer than k candidates -> rows of the last key" rule (F7) describes an unfiltered query and is
        NOT applied to a filtered one, whatever `compat` says.  The candidate counts (and `candidate_budget`) count the rows of the
        probed buckets BEFORE the filter.  Tiled schedule, two-step route (`last_query_path == "two_step"`).
        `tag_mask` / `tag_match` (not in the reference; an index built with `tags=` only): per-query tag filters, see `scan_tensors`; the
        lists and counts follow the rules of a filtered call."""
        filter = self._checked_filter(filter, None, tag_mask, tag_match, query_vectors)
        k1 = self._refine_k1(k, refine_k)
        with _collector_pause if self.pause_collector_for_call else _no_pause:
            if k1 or filter is not None:
                result = self._query_two_step(query_vectors, k, k1, hash_times, seed, probes, candidate_budget, filter)
            elif candidate_budget is not None:
                result = self._query(query_vectors, k, hash_times, seed, self._candidate_budget(candidate_budget, probes))
            elif probes is not None:        # the call again with the mode on the hasher: it keeps its own result
                with self._probe_mode(probes):
                    return self.query(query_vectors, k, hash_times, seed)
            else:
                result = self._query(query_vectors, k, hash_times, seed)
            return self._keep(result)

    def _query(self, query_vectors, k, hash_times, seed, budget=None):
        self.last_query_path = "two_step"
        if self.metric not in ("l2", "cosine"):
            return self._query_generic(query_vectors, k, hash_times)
        q = self._as_queries(query_vectors)
        Q = q.shape[0]
        if hash_times < 1:
            raise ValueError(f"`n` should be positive integer, but got {hash_times}")
        fused = None
        if self._fuses_ranked(q, hash_times, self.choose_algo(Q, hash_times), ranked=True if budget is not None else None):
            # every row range is ranked, looked up and scanned by ONE call (five launches) into its rows of the batch's key table, which is
            # kept per (stream, batch shape): two streams never share one
            keys, nkeys = self._kept_key_table("_ranked_key_tables", (_stream(q.device), q.device, Q, hash_times))
            fused = ("ranked", budget or 0, self._n_multi_rows(Q))
            self.last_query_path = "ranked_one_call"
        elif budget is not None:            # ranked keys cut at the candidate budget, two steps
            keys, nkeys, _ = self._hash_budget(q, HASH_BATCH, hash_times, budget)
        elif self._fuses(q, hash_times, self.choose_algo(Q, hash_times)):
            self.last_query_path = "fused"
            # every row range is hashed and scanned by ONE call (five launches); the ranges share the batch's key table, seed and the
            # Philox counters of its rows, so the split changes no key
            keys, nkeys = self._kept_key_table("_key_tables", (q.device, Q, hash_times))
            fused = (hash_times, self._hashing.next_seed() if seed is None else seed, self._n_multi_rows(Q))
        else:
            keys, nkeys = self.hash_device(q, hash_times=hash_times, seed=seed)
        if keys.shape[1] > _capi.MAX_PROBES:
            _, idx, ncand, _ = self.scan_tensors(q, keys, nkeys, k=k, refine_k=0)
            idx_h, nc_h = idx.cpu().numpy(), ncand.cpu().numpy()
            keys_h, nkeys_h = (keys.cpu().numpy(), nkeys.cpu().numpy()) if self.compat else (None, None)
            return self._to_lists(self._short_key_sets(nc_h, keys_h, nkeys_h, k), idx_h, nc_h, k)
        # the containers (`shells`, where the two-phase construction runs) are built while the device scans: between the launch and the
        # stream synchronisation of a single range, while range 1 scans of several -- whose ids then land as each range's event completes
        shells, chunks = self._shells(Q, k), self._n_chunks()
        queued = None if shells is None else shells.alloc
        if chunks > 1 and Q >= chunks * self._CHUNK_MIN_ROWS:
            ranges = self._chunked_results(q, keys, nkeys, k, chunks, fused, queued)
        else:                           # one range in the shape of several: a tuple, no generator on the default path
            ranges = ((0, Q) + self._host_results(q, keys, nkeys, k, fused, queued),)
        if shells is not None:
            for lo, hi, idx_h, nc_h, keys_h, nkeys_h in ranges:
                self._fill_range(shells, lo, hi, idx_h, nc_h, keys_h, nkeys_h, k)
            return shells.rows, shells.counts
        results = counts = None
        for _, _, idx_h, nc_h, keys_h, nkeys_h in ranges:
            r, c = self._to_lists(self._short_key_sets(nc_h, keys_h, nkeys_h, k), idx_h, nc_h, k)
            if results is None:         # the first range's lists are the result's: a single range is handed on as it was built
                results, counts = r, c
            else:
                results += r
                counts += c
        return results, counts

    def _kept_key_table(self, cache, ckey):
        """The (keys [Q, P], nkeys [Q]) table `query()` keeps per batch shape in the dictionary named `cache` (`_key_tables`: the fused
        form, `_ranked_key_tables`: the ranked one-call form, per stream as well -- the two never share a table); `ckey` ends in
        (device, Q, P).  The table is consumed inside the call (pinned copy for the F7 rule); a caller sweeping shapes keeps at most nine."""
        tab = self.__dict__.setdefault(cache, {})
        got = tab.get(ckey)
        if got is None:
            if len(tab) > 8:
                tab.clear()
            dev, Q, P = ckey[-3:]
            got = tab[ckey] = (torch.empty((Q, P), dtype=torch.int32, device=dev), torch.empty((Q,), dtype=torch.int32, device=dev))
        return got

    def _short_key_sets(self, nc_h, keys_h, nkeys_h, k):
        """{query: its key set} for the queries with < k candidates: F7 (compat) needs their key SETS (Python iteration order) only."""
        if not self.compat:
            return {}
        return {qi: host_key_set(keys_h[qi], int(nkeys_h[qi]), self._hashing.key_mode) for qi in np.nonzero(nc_h < k)[0].tolist()}

    def _as_queries(self, query_vectors):
        q = query_vectors
        if q.device.type != "cuda":
            raise _capi.NlshHipError(_capi.E_INVALID, "queries must be device-resident; there is no CPU path")
        if q.dtype != torch.float32 or q.stride(1) != 1:
            q = q.float().contiguous()
        return q

    @staticmethod
    def _pack_key_lists(key_lists, dev):
        """Caller-supplied key lists -> (the lists de-duplicated, keys int32 [Q, P] and nkeys int32 [Q] on `dev`).  A query's keys are a
        set (nlsh/utils.pyx:27-31): a repeated key probes its bucket once, first-occurrence order kept; the table is padded to the
        longest list (P >= 1) and holds keys >= 2^31 as the same 32 bits, signed."""
        key_lists = [list(dict.fromkeys(int(key) for key in ks)) for ks in key_lists]
        Q = len(key_lists)
        P = max([len(ks) for ks in key_lists] + [1])
        tab = np.zeros((Q, P), dtype=np.int64)
        cnt = np.zeros((Q,), dtype=np.int32)
        for i, ks in enumerate(key_lists):
            cnt[i] = len(ks)
            tab[i, :len(ks)] = ks
        tab = np.where(tab >= (1 << 31), tab - (1 << 32), tab).astype(np.int32)
        return key_lists, torch.as_tensor(tab).to(dev), torch.as_tensor(cnt).to(dev)

    def query_with_keys(self, query_vectors, key_lists: Sequence[Sequence[int]], k=10, filter=None, refine_k=None, tag_mask=None,
                        tag_match="any"):
        """Scan stage on caller-supplied key lists (each in the iteration order the caller saw):
        parity on identical candidate sets, independent of hashing.  `filter`: as in `query` (allowed ids only, list lengths
        from the sort keys, no F7 rule, candidate counts before the filter).  `tag_mask` / `tag_match`: as in `query`."""
        filter = self._checked_filter(filter, None, tag_mask, tag_match, query_vectors)
        self._refine_k1(k, refine_k)        # refused before anything is copied to the device
        key_lists, keys, nkeys = self._pack_key_lists(key_lists, query_vectors.device)
        if filter is not None:
            dist, idx, ncand, keys64 = self.scan_tensors(query_vectors, keys, nkeys, k=k, want_keys=True, filter=filter, refine_k=refine_k)
            return self._filtered_lists(idx, ncand, keys64) + (dist, idx)
        dist, idx, ncand, _ = self.scan_tensors(query_vectors, keys, nkeys, k=k, refine_k=refine_k)
        res, nc = self._to_lists(key_lists, idx.cpu().numpy(), ncand.cpu().numpy(), k)
        return res, nc, dist, idx

    def _global_ids(self, local_rows):
        return self.row_ids[local_rows].long() if self.row_ids is not None else local_rows + self.id_base

    def _query_generic(self, query_vectors, k, hash_times):
        """Arbitrary distance callable: the reference's gather -> callable -> topk per query
        (indexer.py:62-95) on the CSR index, with stock device ops.  Not accelerated."""
        key_sets = self.hash(query_vectors, hash_times=hash_times)
        results, n_candidates = [], []
        corpus = self._candidate_vectors_gpu
        for qi, ks in enumerate(key_sets):
            chunks, last = [], None
            for key in list(ks):
                kk = int(key) - (1 << 32) if int(key) >= (1 << 31) else int(key)
                i = int(np.searchsorted(self._uniq_host, kk))
                last = None                                          # indexer.py:68,92: the last key's rows, [] if it has no bucket
                if i < len(self._uniq_host) and int(self._uniq_host[i]) == kk:
                    last = self.perm[int(self._offs_host[i]):int(self._offs_host[i + 1])].long()
                    chunks.append(last)
            rows = torch.cat(chunks) if chunks else torch.zeros((0,), dtype=torch.int64, device=corpus.device)
            n_candidates.append(int(rows.numel()))
            if rows.numel() >= k:
                # a compressed index answers from the rows as it holds them (the caller's corpus may be un-rounded float32)
                dist = self._distance_func(query_vectors[qi], self._dequantised(corpus[rows]) if self.compressed else corpus[rows])
                results.append(self._global_ids(rows[dist.topk(k, largest=False)[1]]).tolist())
            elif self.compat:
                results.append([] if last is None else self._global_ids(last).tolist())
            else:
                results.append(self._global_ids(rows).tolist())
        return results, n_candidates
