"""Exact brute-force k-NN on the device (nlsh_exact_topk, csrc/exact_knn.hip): ground truth for recall figures and the self-kNN the
triplet recipe trains on (the reference's precompute.py:22-67), without a [chunk, N] distance matrix.

Distances are precompute.py's forms -- squared L2 `(|c|^2 - 2 q.c) + |q|^2`, cosine `1 - q.c / (|q| |c|)` with norms clamped at 1e-12 --
each dot product one fp32 chain over the dimension; lists are ordered by (distance bits, row id).  Inputs must be finite.  There is no CPU
path: anything but device-resident float32 matrices raises `NlshHipError(E_INVALID)`.
"""
import torch

from . import _capi
from ._capi import NlshHipError

Q_CHUNK = 65536                      # queries per native call: bounds the workspace at 4 N + O(splits * Q_CHUNK * k) bytes
_METRICS = {"l2": _capi.EXACT_L2, "cosine": _capi.EXACT_COSINE}
_workspaces = {}                     # (device index, stream handle) -> uint8 tensor, grown on demand


def _matrix(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NlshHipError(_capi.E_INVALID, f"exact_topk: {name} must be a device-resident torch tensor (there is no CPU path)")
    if t.dtype != torch.float32 or t.dim() != 2:
        raise NlshHipError(_capi.E_INVALID, f"exact_topk: {name} must be a float32 matrix, got {t.dtype} with {t.dim()} dimensions")
    rows, d = t.shape   # strides of an empty or one-row matrix carry no meaning
    if (rows > 0 and d > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < d):
        raise NlshHipError(_capi.E_INVALID, f"exact_topk: {name} needs unit column stride and a row stride >= d (strides {t.stride()})")
    return t


def _row_stride(t):
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _workspace(device, stream, nbytes):
    key = (device.index, stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        _workspaces[key] = ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    return ws


def workspace_bytes(Q, N, k, splits=None):
    """Bytes one native call on min(Q, Q_CHUNK) queries takes (what exact_topk keeps per stream)."""
    return int(_capi.lib().nlsh_exact_workspace(min(int(Q), Q_CHUNK), int(N), int(k), int(splits or 0)))


def exact_topk(queries, corpus, k, metric="l2", self_row0=None, splits=None):
    """(dist float32 [Q, k], idx int32 [Q, k]) of the k nearest corpus rows of every query, ascending by (distance, row id); with fewer
    than k eligible rows the tail is idx -1 / dist +inf.  Row views with a row stride are passed through without a copy.
    self_row0: query i skips corpus row self_row0 + i (self-kNN of rows self_row0.. of `corpus`; excluded by id, where the reference
    drops column 0 of a k+1 list and so may keep a row and drop its exact duplicate).  splits: column splits of the corpus (None =
    automatic); results do not depend on it, bit for bit."""
    queries, corpus = _matrix(queries, "queries"), _matrix(corpus, "corpus")
    if metric not in _METRICS:
        raise NlshHipError(_capi.E_INVALID, f"exact_topk: metric {metric!r} is neither 'l2' nor 'cosine'")
    if queries.device != corpus.device or queries.shape[1] != corpus.shape[1]:
        raise NlshHipError(_capi.E_INVALID, f"exact_topk: queries {tuple(queries.shape)} on {queries.device} against corpus "
                                            f"{tuple(corpus.shape)} on {corpus.device}")
    L = _capi.lib()
    Q, d = queries.shape
    N, k, splits = corpus.shape[0], int(k), int(splits or 0)
    self0 = -1 if self_row0 is None else int(self_row0)
    if self_row0 is not None and self0 < 0:
        raise NlshHipError(_capi.E_INVALID, f"exact_topk: self_row0={self_row0}")
    dev = queries.device
    with torch.cuda.device(dev):
        dist = torch.empty((Q, max(k, 0)), dtype=torch.float32, device=dev)
        idx = torch.empty((Q, max(k, 0)), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        qs, cs = _row_stride(queries), _row_stride(corpus)
        for s in range(0, max(Q, 1), Q_CHUNK):
            n = min(Q_CHUNK, Q - s)
            need = L.nlsh_exact_workspace(n, N, k, splits)
            ws = _workspace(dev, stream, need) if need else None
            qv = queries[s:s + n]
            _capi.check(L.nlsh_exact_topk(_capi.ptr(corpus), cs, N, d, _capi.ptr(qv), qs, n, k, _METRICS[metric],
                                          self0 + s if self0 >= 0 else -1, splits, _capi.ptr(dist[s:s + n]), _capi.ptr(idx[s:s + n]),
                                          _capi.ptr(ws), ws.numel() if ws is not None else 0, stream))
    return dist, idx


def self_knn(x, k, metric="l2"):
    """Row ids int64 [n, k] of each row's k nearest OTHER rows: the surface of `training.self_knn`, computed by nlsh_exact_topk."""
    return exact_topk(x, x, k, metric=metric, self_row0=0)[1].to(torch.int64)
