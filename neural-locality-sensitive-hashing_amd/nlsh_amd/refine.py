"""Exact re-ranking: a store of the index's ORIGINAL float32 rows in id order and the second stage that rescores a
query's candidates on it (`nlsh_rerank_topk`, csrc/rerank.hip).

A compressed index (`storage="float16"` / `"uint8"` / `"sq8"`) and a folded-L2 index return distances to rows, or in an operation order,
the caller never supplied.  With a `RefineStore` behind it, stage one over-fetches `k1 > k` candidates and stage two returns the k best
of them by the distance bits the tiled float32 scan gives the same (query, row) pair.  The store addresses a row by `id - id_base`, so
the ids of an index that owns one are the contiguous default ones.
"""
import torch

from . import _capi

WHERE = ("device", "host")
MAX_KC = _capi.MAX_K_TILED      # candidates per query one re-rank takes
HOST_CHUNK_ROWS = 1 << 16       # where="host": rows gathered on the device per copy into the pinned store


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def stage_one_k(k, refine_factor, refine_k=None):
    """k1 of a refined call: `refine_k` when given (k <= refine_k <= 256; 0 = the stage is off for this call -> 0), else
    min(256, max(k, refine_factor * k)).  Host arithmetic only."""
    k = int(k)
    if refine_k is None:
        return min(MAX_KC, max(k, int(refine_factor) * k))
    if isinstance(refine_k, bool) or int(refine_k) != refine_k:
        raise ValueError(f"refine_k must be None, 0 or an integer in [k, {MAX_KC}], got {refine_k!r}")
    refine_k = int(refine_k)
    if refine_k == 0:
        return 0
    if refine_k < k:
        raise ValueError(f"refine_k={refine_k} is less than k={k}: stage one must fetch at least the k rows stage two returns")
    if refine_k > MAX_KC:
        raise ValueError(f"refine_k={refine_k}: a re-rank takes at most {MAX_KC} candidates per query (NLSH_MAX_K_TILED)")
    return refine_k


def checked_refine(refine, refine_factor):
    """`refine=` / `refine_factor=` of a constructor, checked before anything touches a device."""
    if refine is not None and refine not in WHERE:
        raise ValueError(f"refine must be None or one of {WHERE}, got {refine!r}")
    if isinstance(refine_factor, bool) or int(refine_factor) != refine_factor or int(refine_factor) < 1:
        raise ValueError(f"refine_factor must be an integer >= 1, got {refine_factor!r}")
    return refine, int(refine_factor)


class RefineStore:
    """Rows [N, d] (device tensor, any dtype `.float()` converts exactly enough for the caller) kept as float32 in id order: row i is the
    row with id `id_base + i`.  `where="device"`: one device tensor [N, pitch].  `where="host"`: one pinned host tensor the kernel reads
    over the host link, filled in bounded chunks (no second full device copy); `inv_norm` (cosine) stays on the device either way.
    The copy is made by `nlsh_gather_rows` with the identity permutation: zero-padded pitch, and `inv_norm` has the gather's bits."""

    def __init__(self, rows, metric, id_base=0, where="device", row_align=4):
        if metric not in ("l2", "cosine"):
            raise NotImplementedError("a refine store needs metric 'l2' or 'cosine': the re-rank kernel computes the distance")
        if where not in WHERE:
            raise ValueError(f"where must be one of {WHERE}, got {where!r}")
        if row_align % 4 or row_align < 4:
            raise ValueError("row_align must be a multiple of 4 floats")
        if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
            raise ValueError("rows must be a [N, d] tensor")
        if rows.device.type != "cuda":
            raise _capi.NlshHipError(_capi.E_INVALID, "a refine store is built from device-resident rows; there is no CPU path")
        self.metric, self.where, self.id_base = metric, where, int(id_base)
        self.dim = int(rows.shape[1])
        if not 1 <= self.dim <= _capi.MAX_DIM:
            raise ValueError(f"d={self.dim}: a refine store takes 1 <= d <= {_capi.MAX_DIM}")
        self.stride = (self.dim + row_align - 1) // row_align * row_align
        self.device = rows.device
        self.rows = self._empty(0)
        self.inv_norm = torch.empty((0,), dtype=torch.float32, device=self.device) if metric == "cosine" else None
        self.append(rows)

    @property
    def n_rows(self):
        return int(self.rows.shape[0])

    def _empty(self, n):
        if self.where == "host":
            return torch.empty((n, self.stride), dtype=torch.float32, pin_memory=True)
        return torch.empty((n, self.stride), dtype=torch.float32, device=self.device)

    def _gather_into(self, src, out, inv):
        """src float32 [M, d] (unit column stride, device) -> out [M, stride] (device), inv [M] | None: nlsh_gather_rows, identity order."""
        M = int(src.shape[0])
        perm = torch.arange(M, dtype=torch.int32, device=self.device)
        _capi.check(_capi.lib().nlsh_gather_rows(_capi.ptr(src), src.stride(0), self.dim, _capi.ptr(perm), M, _capi.ptr(out), self.stride,
                                                 _capi.ptr(inv), None, 0, _stream(self.device)))

    def append(self, rows):
        """Grow the store by rows [M, d] (ids n_rows + id_base ..): allocate-and-copy."""
        if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or int(rows.shape[1]) != self.dim:
            raise ValueError(f"rows must be [M, {self.dim}]")
        if rows.device != self.device:
            raise ValueError(f"rows are on {rows.device}, the store on {self.device}")
        M, N = int(rows.shape[0]), self.n_rows
        if self.id_base + N + M - 1 > 0x7FFFFFFF:
            raise ValueError("row ids are int32: id_base + rows exceeds 2^31 - 1")
        if self.id_base <= -1 < self.id_base + N + M:
            raise ValueError("a refine store cannot hold the row with id -1: -1 is the padding of a candidate list")
        if M == 0:
            return
        grown = self._empty(N + M)
        inv = None
        if self.inv_norm is not None:
            inv = torch.empty((N + M,), dtype=torch.float32, device=self.device)
            inv[:N] = self.inv_norm
        if N:
            grown[:N] = self.rows
        chunk = HOST_CHUNK_ROWS if self.where == "host" else M
        staged = torch.empty((min(chunk, M), self.stride), dtype=torch.float32, device=self.device) if self.where == "host" else None
        for lo in range(0, M, chunk):
            part = rows[lo:lo + chunk]
            if part.dtype != torch.float32:
                part = part.float()
            if part.stride(1) != 1:
                part = part.contiguous()
            m = int(part.shape[0])
            inv_part = None if inv is None else inv[N + lo:N + lo + m]
            if staged is None:
                self._gather_into(part, grown[N + lo:N + lo + m], inv_part)
            else:
                self._gather_into(part, staged[:m], inv_part)
                grown[N + lo:N + lo + m].copy_(staged[:m])      # device -> pinned host, synchronous with the host
        if self.where == "host":
            torch.cuda.current_stream(self.device).synchronize()
        self.rows, self.inv_norm = grown, inv

    def rerank(self, queries, cand, k, want_keys=False, check=True):
        """queries float32 [Q, d] (device, strided row views allowed), cand int32 [Q, kc] (device; -1 = padding) -> (dist [Q, k], idx
        [Q, k], count [Q][, keys64 [Q, k]]): one launch on the current stream.  check=True reads `first_bad` back and raises ValueError
        naming the first query whose list held an id outside the store (such ids are dropped, never read); check=False leaves the
        flag on the device in `last_first_bad` and does not synchronise."""
        if queries.device != self.device or cand.device != self.device:
            raise ValueError(f"queries and cand must be on {self.device}")
        if queries.dtype != torch.float32 or queries.dim() != 2 or queries.stride(1) != 1:
            queries = queries.float().contiguous()
        if cand.dtype != torch.int32 or cand.dim() != 2 or (cand.shape[1] > 1 and cand.stride(1) != 1):
            cand = cand.to(torch.int32).contiguous()
        Q, d = int(queries.shape[0]), int(queries.shape[1])
        if d != self.dim:
            raise ValueError(f"query dim {d} != store dim {self.dim}")
        if int(cand.shape[0]) != Q:
            raise ValueError(f"cand holds {int(cand.shape[0])} lists for {Q} queries")
        kc = int(cand.shape[1])
        dev = self.device
        out_dist = torch.empty((Q, k), dtype=torch.float32, device=dev)
        out_idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
        out_keys = torch.empty((Q, k), dtype=torch.int64, device=dev) if want_keys else None
        flags = torch.empty((Q + 1,), dtype=torch.int32, device=dev)      # count [Q] | first_bad
        count, first_bad = flags[:Q], flags[Q:]
        if Q == 0:
            first_bad.fill_(-1)
        inv = self.inv_norm
        if inv is not None and not self.n_rows:
            inv = torch.zeros((1,), dtype=torch.float32, device=dev)      # an empty store still names its norms (never read)
        _capi.check(_capi.lib().nlsh_rerank_topk(
            _capi.ptr(queries), max(queries.stride(0), d) if Q == 1 else queries.stride(0) if Q else d, Q, d,
            _capi.ptr(self.rows) if self.n_rows else None, self.stride, self.n_rows, self.id_base, int(self.where == "host"),
            _capi.ptr(inv), _capi.ptr(cand), max(cand.stride(0), kc) if Q == 1 else cand.stride(0) if Q else kc, kc, int(k),
            _capi.METRIC_COSINE if self.metric == "cosine" else _capi.METRIC_L2_EPS,
            _capi.ptr(out_dist), _capi.ptr(out_idx), _capi.ptr(out_keys), _capi.ptr(count), _capi.ptr(first_bad), _stream(dev)))
        self.last_first_bad = first_bad
        if check:
            bad = int(first_bad.item())
            if bad >= 0:
                raise ValueError(f"query {bad}: its candidate list holds an id outside the refine store "
                                 f"[{self.id_base}, {self.id_base + self.n_rows}) (such ids were dropped, never read)")
        return (out_dist, out_idx, count, out_keys) if want_keys else (out_dist, out_idx, count)
