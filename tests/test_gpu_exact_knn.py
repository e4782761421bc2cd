"""nlsh_exact_topk on the device (csrc/exact_knn.hip, nlsh_amd/exact.py): exact brute-force k-NN with fp32-MFMA distances and the top-k
fused behind them.  The reference is float64 numpy computed here -- never the code under test, never torch.topk.  Every test fails on a
library without the two nlsh_exact_* symbols.

Rounding bound B of the implemented forms (u = 2^-24; every chain is an fmaf chain of d terms, |chain - exact| <= g sum|a_i b_i| with
g = d u / (1 - d u)):
  L2      D^ = fl(fl(cn^ - 2 dot^) + qn^).  |cn^ - |c|^2| <= g |c|^2, |qn^ - |q|^2| <= g |q|^2, |2 dot^ - 2 q.c| <= 2 g |q||c| <=
          g (|q|^2 + |c|^2): 2 g (|q|^2 + |c|^2) from the inputs.  The first rounding acts on |t| <= |c|^2 + 2 |q||c| <= 2 (|q|^2 + |c|^2),
          the second on D <= (|q| + |c|)^2 <= 2 (|q|^2 + |c|^2): 2 u (|q|^2 + |c|^2) each (2 x is exact).  Sum (2 d + 4) u (|q|^2 + |c|^2) up to
          a factor 1 + O(d u) <= 1 + 2^-13, inside  B = 2 (d + 3) u (|q|^2 + |c|^2)  for d <= 1024.
  cosine  D^ = fl(1 - fl(fl(dot^ iq^) ic^)), iq^ = fl(1 / max(fl(sqrt(ss^)), 1e-12)).  ss^ has relative error g (positive terms), the root
          halves it and adds u, the reciprocal adds u: iq^ = iq (1 + e), |e| <= d u / 2 + 2 u.  |dot^ - q.c| iq ic <= g.  Two products: 2 u.
          |cos| <= 1, so the cosine carries d u + 2 (d u / 2 + 2 u) + 2 u = (2 d + 6) u, the subtraction rounds a value <= 2: 2 u more.
          (2 d + 8) u up to 1 + O(d u), inside  B = 2 (d + 8) u.  A zero vector has iq^ = 1e12 and dot^ = 0 exactly: D^ = 1 = D.
With t the k-th smallest float64 distance of a query and Bq the largest B over its rows: the k rows at or below t have D^ <= t + Bq, so a
returned row has D^ <= t + Bq and D64 <= t + 2 Bq; a row with D64 < t - 2 Bq has D^ < t - Bq <= the D^ of at least N - k + 1 rows, so it
is returned."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nlsh_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(q, c, k, **kw):
    from nlsh_amd import exact
    dist, idx = exact.exact_topk(q if torch.is_tensor(q) else _dev(q), c if torch.is_tensor(c) else _dev(c), k, **kw)
    torch.cuda.synchronize()
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32 and dist.shape == idx.shape == (q.shape[0], k)
    return dist.cpu().numpy(), idx.cpu().numpy()


def _d64(q, c, metric):
    q, c = q.astype(np.float64), c.astype(np.float64)
    if metric == "l2":
        # in float64 the expanded form is exact on the integer data and within 1e-15 (|q|^2 + |c|^2) of |q - c|^2 otherwise: nothing beside B
        return ((q * q).sum(1)[:, None] - 2.0 * (q @ c.T)) + (c * c).sum(1)[None, :]
    qn, cn = np.maximum(np.linalg.norm(q, axis=1), 1e-12), np.maximum(np.linalg.norm(c, axis=1), 1e-12)
    return 1.0 - (q @ c.T) / qn[:, None] / cn[None, :]


def _bound(q, c, metric):
    d = q.shape[1]
    if metric == "l2":
        q, c = q.astype(np.float64), c.astype(np.float64)
        return 2.0 * (d + 3) * U * ((q * q).sum(1)[:, None] + (c * c).sum(1)[None, :])
    return np.full((q.shape[0], c.shape[0]), 2.0 * (d + 8) * U)


def _mono(dist):
    u = np.ascontiguousarray(dist, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def _check_against_fp64(dist, idx, D, B, k, skip_self0=None):
    """Condition (5) of the module docstring for EVERY query.  skip_self0: query i may not list row skip_self0 + i (D holds +inf there)."""
    Q, N = D.shape
    kk = min(k, N - (0 if skip_self0 is None else 1))
    assert (idx[:, kk:] == -1).all() and np.isposinf(dist[:, kk:]).all()
    ids = idx[:, :kk].astype(np.int64)
    assert (ids >= 0).all() and (ids < N).all()
    srt = np.sort(ids, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "repeated ids"
    keys = (_mono(dist[:, :kk]) << np.uint64(32)) | ids.astype(np.uint64)
    assert (keys[:, 1:] > keys[:, :-1]).all(), "lists are not ascending in (distance bits, id)"
    if skip_self0 is not None:
        assert (ids != (skip_self0 + np.arange(Q))[:, None]).all(), "a row lists itself"
    Bq = np.where(np.isfinite(D), B, 0.0).max(axis=1)
    t = np.partition(D, kk - 1, axis=1)[:, kk - 1]
    got = np.take_along_axis(D, ids, axis=1)
    worst = (got - (t + 2 * Bq)[:, None]).max()
    assert worst <= 0, f"a returned row lies {worst} beyond t + 2B"
    err = np.abs(dist[:, :kk].astype(np.float64) - got) - np.take_along_axis(B, ids, axis=1)
    assert err.max() <= 0, f"a returned distance is {err.max()} beyond B of its float64 value"
    member = np.zeros((Q, N), dtype=bool)
    np.put_along_axis(member, ids, True, axis=1)
    must = D < (t - 2 * Bq)[:, None]
    assert not (must & ~member).any(), "a row more than 2B inside the k-th distance is missing"


# ------------------------------------------------------------------------------------------------ 1. bit-exact on integer data
def _int_data(n, d, seed):
    return np.random.default_rng(seed).integers(0, 16, size=(n, d)).astype(np.float32)


def _exact_reference(q, c):
    """ids sorted by (float64 distance, id) and the distances, for all N rows: products and sums are integers < 2^24."""
    D = _d64(q, c, "l2")
    order = np.stack([np.lexsort((np.arange(c.shape[0]), row)) for row in D])
    return order, np.take_along_axis(D, order, axis=1)


@pytest.mark.parametrize("d", [1, 3, 96, 100, 128, 130, 1024])
def test_integer_data_is_bit_exact(d):
    c = _int_data(1037, d, 100 + d)
    cg = _dev(c)
    for Q in (1, 129, 200):
        q = _int_data(Q, d, 200 + d + Q)
        order, dsorted = _exact_reference(q, c)
        qg = _dev(q)
        for k in (1, 10, 64, 65, 100, 256):
            dist, idx = _run(qg, cg, k)
            assert np.array_equal(idx, order[:, :k].astype(np.int32)), (d, Q, k)
            assert np.array_equal(dist, dsorted[:, :k].astype(np.float32)), (d, Q, k)


def test_integer_data_many_tiles():
    """157 corpus tiles per query tile: all but the first few are filtered by the running threshold."""
    c, q = _int_data(20000, 100, 7), _int_data(300, 100, 8)
    order, dsorted = _exact_reference(q, c)
    for splits in (1, None):
        dist, idx = _run(q, c, 100, splits=splits)
        assert np.array_equal(idx, order[:, :100].astype(np.int32))
        assert np.array_equal(dist, dsorted[:, :100].astype(np.float32))


# ------------------------------------------------------------------------------------------------ 2. mass ties
@pytest.mark.parametrize("k", [10, 256])
def test_mass_ties_break_by_row_id(k):
    rng = np.random.default_rng(5)
    c = np.repeat(rng.standard_normal((1, 32)).astype(np.float32), 2000, axis=0)
    q = rng.standard_normal((64, 32)).astype(np.float32)
    for metric in ("l2", "cosine"):
        for splits in (1, 3, None):
            dist, idx = _run(q, c, k, metric=metric, splits=splits)
            assert np.array_equal(idx, np.tile(np.arange(k, dtype=np.int32), (64, 1))), (metric, splits)
            assert (dist == dist[:, :1]).all()
            _, idx = _run(c[:64], c, k, metric=metric, splits=splits, self_row0=0)
            want = np.stack([[r for r in range(k + 1) if r != i][:k] for i in range(64)]).astype(np.int32)
            assert np.array_equal(idx, want), (metric, splits)


# ------------------------------------------------------------------------------------------------ 3. fewer rows than k
def test_fewer_rows_than_k():
    c, q = _int_data(5, 16, 1), _int_data(7, 16, 2)
    order, dsorted = _exact_reference(q, c)
    dist, idx = _run(q, c, 10)
    assert np.array_equal(idx[:, :5], order.astype(np.int32)) and (idx[:, 5:] == -1).all()
    assert np.array_equal(dist[:, :5], dsorted.astype(np.float32)) and np.isposinf(dist[:, 5:]).all()
    dist, idx = _run(q, np.zeros((0, 16), np.float32), 10)
    assert (idx == -1).all() and np.isposinf(dist).all()
    from nlsh_amd import exact
    dist, idx = exact.exact_topk(_dev(q)[:0], _dev(c), 10)
    assert dist.shape == idx.shape == (0, 10)


# ------------------------------------------------------------------------------------------------ 4. independence of launch shape
@pytest.fixture(scope="module")
def glove():
    c = synth.glove_manifold(6000, 100)
    q = synth.glove_manifold(257, 100, seed=synth.SEED_QUERY)
    return c, q


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("k", [10, 100])
def test_results_do_not_depend_on_splits_or_strides(glove, metric, k):
    c, q = glove
    cg, qg = _dev(c), _dev(q)
    d0, i0 = _run(qg, cg, k, metric=metric, splits=1)
    for splits in (2, 3, 7, None):
        d1, i1 = _run(qg, cg, k, metric=metric, splits=splits)
        assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32)), splits
    wide = torch.full((c.shape[0], 104), 7.0, device="cuda")
    wide[:, :100] = cg
    d1, i1 = _run(qg, wide[:, :100], k, metric=metric)
    assert wide[:, :100].stride(0) == 104
    assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    qwide = torch.full((2 * q.shape[0], 108), -3.0, device="cuda")
    qwide[::2, :100] = qg
    qv = qwide[::2, :100]
    assert qv.stride(0) == 216 and qv.shape == qg.shape
    d1, i1 = _run(qv, cg, k, metric=metric)
    assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 5. continuous data against float64
@pytest.mark.parametrize("k", [10, 100])
def test_l2_against_fp64(k):
    c, q = synth.sift_manifold(8000, 128), synth.sift_manifold(200, 128, seed=synth.SEED_QUERY)
    dist, idx = _run(q, c, k)
    _check_against_fp64(dist, idx, _d64(q, c, "l2"), _bound(q, c, "l2"), k)
    cs, mean, std = synth.standardise(c)          # the same rows as real numbers
    qs, _, _ = synth.standardise(q, mean, std)
    dist, idx = _run(qs, cs, k)
    _check_against_fp64(dist, idx, _d64(qs, cs, "l2"), _bound(qs, cs, "l2"), k)


@pytest.mark.parametrize("k", [10, 100])
def test_cosine_against_fp64_with_zero_vectors(glove, k):
    c, q = glove[0].copy(), glove[1].copy()
    c[1234] = 0.0          # the norm clamp: distance 1 to everything
    q[77] = 0.0
    dist, idx = _run(q, c, k, metric="cosine")
    D = _d64(q, c, "cosine")
    assert (D[77] == 1.0).all() and (D[:, 1234] == 1.0).all()
    _check_against_fp64(dist, idx, D, _bound(q, c, "cosine"), k)
    assert (dist[77] == 1.0).all() and np.array_equal(idx[77], np.arange(k, dtype=np.int32))


# ------------------------------------------------------------------------------------------------ 6. self-kNN
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_self_knn(metric):
    from nlsh_amd import exact
    x = synth.glove_manifold(5000, 100)
    xg = _dev(x)
    knn = exact.self_knn(xg, 10, metric=metric)
    assert knn.dtype == torch.int64 and knn.shape == (5000, 10)
    dist, idx = _run(xg, xg, 10, metric=metric, self_row0=0)
    assert np.array_equal(knn.cpu().numpy(), idx.astype(np.int64))
    D = _d64(x, x, metric)
    np.fill_diagonal(D, np.inf)
    _check_against_fp64(dist, idx, D, _bound(x, x, metric), 10, skip_self0=0)
    d1, i1 = _run(xg[1000:1300], xg, 10, metric=metric, self_row0=1000)
    assert np.array_equal(i1, idx[1000:1300]) and np.array_equal(d1.view(np.uint32), dist[1000:1300].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 7. the tool, end to end
def test_precompute_tool_writes_train_knn(tmp_path):
    from nlsh_amd import data, exact, io
    rng = np.random.default_rng(11)
    base = rng.standard_normal((3000, 32)).astype(np.float32)
    io.write_vecs(str(tmp_path / "toy_base.fvecs"), base)
    io.write_vecs(str(tmp_path / "toy_query.fvecs"), base[:10] + np.float32(0.01))
    io.write_vecs(str(tmp_path / "toy_groundtruth.ivecs"), np.zeros((10, 5), np.int32))
    tool = os.path.join(ROOT, "tools", "precompute_knn.py")
    r = subprocess.run([sys.executable, tool, "--dataset", str(tmp_path), "--k", "20"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "toy_train_knn.ivecs").exists()
    ds = data.SIFT(str(tmp_path))
    ds.load()
    knn = np.asarray(ds.training_self_knn)
    assert knn.shape == (3000, 20)
    assert np.array_equal(knn.astype(np.int64), exact.self_knn(_dev(base), 20).cpu().numpy())
