"""The rule of storage="pq" (include/nlsh_hip.h) in numpy float32: the code the HIP kernels are held against.

A codebook C is float32 [M, 256, dsub], M = ceil(d / dsub).  Every arithmetic step below is one float32 operation on float32 arrays, so
it rounds where the rule says it rounds: a subtract, a multiply and an add per column, ascending over the sub-vector's columns below d."""
import numpy as np


def n_sub(d, dsub):
    return (d + dsub - 1) // dsub


def zero_tail(C, d):
    """The codebook with the columns of the last sub-vector at or beyond d held as +0 (what the library does on intake)."""
    C = np.array(C, dtype=np.float32)
    M, _, dsub = C.shape
    tail = M * dsub - d
    if tail:
        C[M - 1, :, dsub - tail:] = 0.0
    return C


def pq_scores(X, C, d, m):
    """float32 [n, 256]: s(c) of sub-vector m for every row -- acc = 0; for j ascending: t = x_j - C[m][c][j]; acc = acc + t * t."""
    X = np.asarray(X, dtype=np.float32)
    dsub = C.shape[2]
    acc = np.zeros((X.shape[0], 256), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(m * dsub, min(d, (m + 1) * dsub)):
            t = X[:, j, None] - C[m, :, j - m * dsub][None, :]
            acc = acc + t * t
    assert acc.dtype == np.float32
    return acc


def pq_encode(X, C, d):
    """-> (codes uint8 [n, M], first_bad): per sub-vector the lowest index of the smallest score; first_bad = the smallest row that holds a
    NaN or an infinity (-1: none; such a row's codes mean nothing)."""
    X = np.asarray(X, dtype=np.float32)
    M = C.shape[0]
    codes = np.zeros((X.shape[0], M), dtype=np.uint8)
    for m in range(M):
        codes[:, m] = np.argmin(pq_scores(X, C, d, m), axis=1)       # argmin names the FIRST minimum: ties go to the lowest index
    bad = np.flatnonzero(~np.isfinite(X[:, :d]).all(axis=1))
    return codes, (int(bad[0]) if len(bad) else -1)


def pq_decode(codes, C, d):
    """float32 [n, d]: element j is C[j // dsub][code[j // dsub]][j % dsub] -- a copy."""
    codes = np.asarray(codes)
    M, _, dsub = C.shape
    out = np.concatenate([C[m, codes[:, m].astype(np.int64)] for m in range(M)], axis=1)
    return np.ascontiguousarray(out[:, :d], dtype=np.float32)


def brute_f64(X, C, d):
    """The argmin in float64, for data on which float32 is exact: codes uint8 [n, M], lowest index on ties."""
    X = np.asarray(X, dtype=np.float64)
    M, _, dsub = C.shape
    codes = np.zeros((X.shape[0], M), dtype=np.uint8)
    for m in range(M):
        cols = slice(m * dsub, min(d, (m + 1) * dsub))
        diff = X[:, None, cols] - C[m][None, :, :cols.stop - cols.start].astype(np.float64)
        codes[:, m] = np.argmin((diff * diff).sum(-1), axis=1)
    return codes
