"""pq corpus storage against ITS DEFINITION: with S the stored codes, C the codebook and R = decode(S, C), `Indexer(hashing, corpus, dist,
storage="pq")` is, word for word, the float32 index over R -- every index array, every distance bit, id, candidate count and result
list.  The reference is always code that is not under test: the numpy rule (tests/pq_ref.py) for the encoder, a torch gather on the CPU
for the decoder, and the existing float32 path (`algo="tiled"` forced on the twin) on R with the same `corpus_keys=` for the index.
Every comparison but those of the last two tests is `torch.equal` / `array_equal` on raw bits: no tolerance."""
import numpy as np
import pytest
import torch

import multi_table_ref as MT
import pq_ref
from helpers import dev, make_hashing
from helpers import task_table as _task_table
from nlsh_amd import _capi, synth
from test_gpu_corpus_storage import INDEX_ARRAYS, SD, SQ, _dist, _same, assert_same_results
from test_gpu_sq8_storage import _hasher, _shape_world, real_rows, views_of

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- helpers
def sample_codebook(X, d, dsub, rng, noise=0.05):
    """A plausible codebook without training: 256 rows of X per sub-space, jittered; float32 [M, 256, dsub], tail columns zero."""
    M = pq_ref.n_sub(d, dsub)
    P = np.zeros((X.shape[0], M * dsub), np.float32)
    P[:, :d] = X
    C = np.stack([P[rng.integers(0, X.shape[0], 256), m * dsub:(m + 1) * dsub] for m in range(M)]).astype(np.float32)
    C = (C + noise * rng.standard_normal(C.shape)).astype(np.float32)
    return pq_ref.zero_tail(C, d)


def cpu_decode(codes, C, d):
    """torch on the CPU: C[m, codes[:, m]] side by side, the first d columns."""
    codes, C = torch.as_tensor(codes), torch.as_tensor(C)
    return torch.cat([C[m][codes[:, m].long()] for m in range(C.shape[0])], dim=1)[:, :d].contiguous()


def c_encode(rows, C, d, code, pitch=None):
    """`nlsh_pq_encode` itself -> (codes [n, pitch] uint8, pre-filled with 0xAB, first_bad)."""
    n, M, dsub = int(rows.shape[0]), C.shape[0], C.shape[2]
    pitch = M if pitch is None else pitch
    codes = torch.full((n, pitch), 0xAB, dtype=torch.uint8, device="cuda")
    bad = torch.zeros((1,), dtype=torch.int32, device="cuda")
    _capi.check(_capi.lib().nlsh_pq_encode(_capi.ptr(rows), code, rows.stride(0) if n else d, d, n, _capi.ptr(C), dsub, _capi.ptr(codes), pitch,
                                           _capi.ptr(bad), torch.cuda.current_stream().cuda_stream))
    return codes, int(bad.item())


def stored_codes(ix):
    """The codes the index holds, un-permuted to the caller's order, on the CPU."""
    M = ix._store_dim
    codes = torch.empty((ix.gid.shape[0], M), dtype=torch.uint8)
    codes[ix.perm.long().cpu()] = ix.corpus_sorted[:, :M].cpu()
    return codes


def build_pair(hashing, source, dsub, metric="l2", keys=None, codebook=None, row_align=4, **kw):
    """(pq index built from `source`, its float32 twin built from R = the CPU decode of the stored codes), same keys, the twin on the
    tiled schedule."""
    from nlsh_amd.indexer import Indexer
    ck = None if keys is None else dev(np.asarray(keys, np.int32))
    typed = Indexer(hashing, source, _dist(metric), storage="pq", pq_dsub=dsub, quantiser=codebook, row_align=row_align, corpus_keys=ck, **kw)
    codes = stored_codes(typed)
    R = cpu_decode(codes, typed.codebook.cpu(), typed.dim)
    twin = Indexer(hashing, R.cuda(), _dist(metric), algo="tiled", row_align=row_align, corpus_keys=ck, **kw)
    return typed, twin, codes, R


def assert_is_the_twin(typed, twin, cells=(64, 256)):
    d, M = typed.dim, typed._store_dim
    assert typed.storage == "pq" and typed.corpus_sorted.dtype == torch.uint8 and twin.corpus_sorted.dtype == torch.float32
    assert M == pq_ref.n_sub(d, typed.pq_dsub) and typed.row_stride % 16 == 0 and typed.row_stride >= M
    assert tuple(typed.codebook.shape) == (M, 256, typed.pq_dsub) and typed.codebook.is_cuda and typed.codebook.dtype == torch.float32
    assert typed.n_buckets == twin.n_buckets
    for name in INDEX_ARRAYS:
        _same(getattr(typed, name), getattr(twin, name), name)
    _same(typed.bucket_order[:typed.n_buckets], twin.bucket_order[:twin.n_buckets], "bucket_order")
    _same(cpu_decode(typed.corpus_sorted[:, :M].cpu(), typed.codebook.cpu(), d), twin.corpus_sorted[:, :d].cpu().contiguous(), "decode(corpus_sorted)")
    _same(typed._dequantised(typed.corpus_sorted[:, :M]), twin.corpus_sorted[:, :d].contiguous(), "_dequantised(corpus_sorted)")
    assert not bool((typed.corpus_sorted[:, M:] != 0).any()), "padding code bytes are stored as 0"
    if typed.n_buckets:
        for w in cells:
            ct, cw = typed.cells(w), twin.cells(w)
            assert ct[3] == cw[3]
            for i in range(3):
                _same(ct[i], cw[i], f"cells({w})[{i}]")
    it, iw = typed.index2row, twin.index2row
    assert list(it) == list(iw)
    for key in it:
        assert torch.equal(it[key], iw[key]), key


# ---------------------------------------------------------------------------------------------- 1. the encoder
@pytest.mark.parametrize("dsub", [4, 8, 16])
@pytest.mark.parametrize("d", [1, 4, 12, 100, 128, 260, 1024])
def test_encode_equals_the_numpy_rule(d, dsub):
    n = 300
    rng = np.random.default_rng(1000 * d + dsub)
    X = real_rows(n, d, rng)
    C = sample_codebook(X, d, dsub, rng)
    Cd = dev(C)
    M = C.shape[0]
    for dtype, code in ((torch.float32, _capi.STORE_F32), (torch.float16, _capi.STORE_F16)):
        Xs = torch.from_numpy(X).to(dtype).float().numpy()                         # the rows as the source holds them
        want, bad = pq_ref.pq_encode(Xs, C, d)
        assert bad == -1
        for name, src in views_of(X, dtype).items():
            got, first_bad = c_encode(src, Cd, d, code)
            assert first_bad == -1, (dtype, name)
            assert np.array_equal(got.cpu().numpy(), want), (d, dsub, dtype, name)
    # a wider code pitch: only the M code bytes of a row are written
    got, _ = c_encode(dev(X), Cd, d, _capi.STORE_F32, pitch=M + 19)
    assert np.array_equal(got[:, :M].cpu().numpy(), pq_ref.pq_encode(X, C, d)[0]) and bool((got[:, M:] == 0xAB).all())


def test_encode_ties_overflow_refusals_and_no_rows():
    from nlsh_amd.indexer import pq_encode
    d, dsub, n = 20, 8, 300
    rng = np.random.default_rng(7)
    M = pq_ref.n_sub(d, dsub)
    # duplicated centroids on integer data: every minimum is a real tie and goes to the lowest index
    C = rng.integers(-30, 31, size=(M, 256, dsub)).astype(np.float32)
    C[:, 9] = C[:, 2]
    C[:, 128:] = C[:, :128]
    C = pq_ref.zero_tail(C, d)
    X = rng.integers(-40, 41, size=(n, d)).astype(np.float32)
    X[:128, :dsub] = C[0, 128:]
    want = pq_ref.brute_f64(X, C, d)
    assert np.array_equal(pq_ref.pq_encode(X, C, d)[0], want) and int(want.max()) < 128
    got, bad = c_encode(dev(X), dev(C), d, _capi.STORE_F32)
    assert bad == -1 and np.array_equal(got.cpu().numpy(), want)
    # all codes equal: a codebook of one repeated centroid
    one = np.repeat(C[:, :1], 256, axis=1)
    assert int(c_encode(dev(X), dev(one), d, _capi.STORE_F32)[0].max()) == 0
    # +- large finite centroids: differences overflow to infinities, sums to +inf, never to a NaN
    big = np.where(rng.random((M, 256, dsub)) < 0.5, -1.0, 1.0).astype(np.float32) * rng.choice([3e38, 2e38, 1e30, 3.0], size=(M, 256, dsub)).astype(np.float32)
    big = pq_ref.zero_tail(big, d)
    Y = (X * np.float32(1e36)).astype(np.float32)
    Y[::2] = X[::2]
    want, bad = pq_ref.pq_encode(Y, big, d)
    assert bad == -1
    got, bad = c_encode(dev(Y), dev(big), d, _capi.STORE_F32)
    assert bad == -1 and np.array_equal(got.cpu().numpy(), want)
    # a NaN row and an inf row are refused by number, the smallest first
    for value, rows in ((np.nan, (211, 57)), (np.inf, (299, 120)), (-np.inf, (0,))):
        Z = X.copy()
        for r in rows:
            Z[r, (7 * r) % d] = value
        assert c_encode(dev(Z), dev(C), d, _capi.STORE_F32)[1] == min(rows) == pq_ref.pq_encode(Z, C, d)[1]
        assert c_encode(dev(Z).half(), dev(C), d, _capi.STORE_F16)[1] == min(rows)
        with pytest.raises(ValueError, match=rf"corpus row {1000 + min(rows)} holds a NaN or an infinity.*storage='pq'"):
            pq_encode(dev(Z), dev(C), d, "corpus", 1000)
    # no rows
    got, bad = c_encode(torch.empty((0, d), device="cuda"), dev(C), d, _capi.STORE_F32)
    assert bad == -1 and tuple(got.shape) == (0, M)
    assert tuple(pq_encode(torch.empty((0, d), device="cuda"), dev(C), d).shape) == (0, M)


# ---------------------------------------------------------------------------------------------- 2. decode and inv_norm
@pytest.mark.parametrize("d, dsub", [(1, 4), (12, 8), (100, 8), (100, 16), (128, 8), (260, 16), (1024, 4)])
def test_decode_and_inv_norm_equal_the_float32_path(d, dsub):
    from nlsh_amd.indexer import Indexer, pq_decode
    n = 700
    rng = np.random.default_rng(d + dsub)
    X = real_rows(n, d, rng)
    C = sample_codebook(X, d, dsub, rng)
    M = C.shape[0]
    codes = rng.integers(0, 256, size=(n, M)).astype(np.uint8)
    codes[0], codes[1] = 0, 255
    R = cpu_decode(codes, C, d)
    assert np.array_equal(R.numpy().view(np.int32), pq_ref.pq_decode(codes, C, d).view(np.int32))
    wide = torch.zeros((n, M + 21), dtype=torch.uint8, device="cuda")
    wide[:, 3:M + 3] = dev(codes)
    for src in (dev(codes), wide[:, 3:M + 3]):
        _same(pq_decode(src, dev(C), d).cpu(), R, (d, dsub, "decode"))
    # inv_norm: the float32 cosine index over the decoded rows states the rule
    keys = dev(rng.integers(0, 9, size=n).astype(np.int32))
    twin = Indexer(_hasher(d), R.cuda(), _dist("cosine"), algo="tiled", corpus_keys=keys)
    inv = torch.full((n,), 7.0, device="cuda")
    _capi.check(_capi.lib().nlsh_pq_inv_norm(_capi.ptr(wide[:, 3:]), wide.stride(0), n, _capi.ptr(dev(C)), dsub, d, _capi.ptr(inv),
                                             torch.cuda.current_stream().cuda_stream))
    _same(inv[twin.perm.long()], twin.inv_norm, (d, dsub, "inv_norm"))
    zero = np.zeros_like(C)                                          # a row of zeros: the 1e-8 floor
    _capi.check(_capi.lib().nlsh_pq_inv_norm(_capi.ptr(dev(codes)), M, n, _capi.ptr(dev(zero)), dsub, d, _capi.ptr(inv), torch.cuda.current_stream().cuda_stream))
    assert bool((inv == 1e8).all())


# ---------------------------------------------------------------------------------------------- 3. the twin
@pytest.mark.parametrize("d, dsub", [(4, 4), (4, 8), (100, 4), (100, 16), (128, 8), (260, 4), (260, 8), (1024, 16)])
def test_index_arrays_and_one_batch_equal_the_float32_twins(d, dsub):
    """l2 at the default pitch and cosine (the inv_norm bits) at row_align=32; a trained codebook with keys from the hash of the decoded
    rows, and a given codebook with given keys; float32 and float16 sources, and the codes themselves with the codebook."""
    from nlsh_amd.indexer import Indexer
    N, Q = 2000, 64
    rng = np.random.default_rng(100 + d + dsub)
    X = real_rows(N, d, rng)
    hashing = _hasher(d)
    q = dev(real_rows(Q, d, rng, special=False))
    pool = np.unique(np.r_[hashing.hash_device(q, n=1)[0].reshape(-1).cpu().numpy(), np.arange(100, 104)]).astype(np.int32)
    given = rng.choice(pool, size=N).astype(np.int32)
    C = torch.from_numpy(sample_codebook(X, d, dsub, rng))
    for metric, row_align in (("l2", 4), ("cosine", 32)):
        for keys, codebook, src in ((given, C, dev(X)), (given, C, dev(X).half()), (None, None if d <= 128 else C, dev(X))):
            typed, twin, codes, R = build_pair(hashing, src, dsub, metric=metric, keys=keys, codebook=codebook, row_align=row_align)
            assert_is_the_twin(typed, twin)
            if codebook is not None:
                Xs = src.float().cpu().numpy()
                assert np.array_equal(codes.numpy(), pq_ref.pq_encode(Xs, C.numpy(), d)[0]), "the index holds the rule's codes"
            for k in (10, 100):
                ra = typed.query_tensors(q, k=k, hash_times=4, seed=3)
                assert typed.last_query_path == "two_step" and typed.last_algo == _capi.SCAN_BUCKET_TILED
                assert_same_results(ra, twin.query_tensors(q, k=k, hash_times=4, seed=3), (metric, keys is None, src.dtype, k))
            if keys is not None:
                assert int(ra[2].sum()) > 0
        # a uint8 corpus is codes: with the codebook it is the same index
        again = Indexer(hashing, codes.cuda(), _dist(metric), storage="pq", pq_dsub=dsub, pq_dim=d, row_align=row_align,
                        corpus_keys=typed.corpus_keys, quantiser=typed.codebook)
        for name in INDEX_ARRAYS + ("corpus_sorted",):
            _same(getattr(again, name), getattr(typed, name), ("from codes", name))


def test_keys_come_from_the_decoded_rows_hashed_in_chunks():
    """N > HASH_BATCH: the keys are those of R = decode(encode(X)), hashed HASH_BATCH rows at a time, not of the caller's rows."""
    from nlsh_amd.indexer import HASH_BATCH, Indexer
    d, N = 24, HASH_BATCH + 904
    rng = np.random.default_rng(5)
    X = real_rows(N, d, rng)
    hashing = _hasher(d)
    C = torch.from_numpy(sample_codebook(X, d, 8, rng, noise=0.5))
    typed, twin, _, _ = build_pair(hashing, dev(X), 8, codebook=C)
    assert_is_the_twin(typed, twin, cells=(64,))
    unrounded = Indexer(hashing, dev(X), _dist("l2"), algo="tiled")
    assert not torch.equal(unrounded.corpus_keys, typed.corpus_keys)            # (the quantisation really moves some keys: the test can tell)


@pytest.mark.parametrize("form, dsub", [("l2", 8), ("l2", 4), ("folded", 16), ("cosine", 8)])
def test_scan_equals_the_twin_on_every_task_shape(form, dsub):
    """d = 100: dsub 4 divides it, 8 and 16 leave a partial last sub-vector.  The bucket world of the sq8 test: every (queries of a wave,
    tiles) shape, the single-stage body either side of its 1024-slot threshold, shared windows, a bucket of identical rows (equal codes)."""
    metric = "cosine" if form == "cosine" else "l2"
    X, corpus_keys, buckets, keys, nkeys, q = _shape_world(seed=11 + len(form))
    rng = np.random.default_rng(dsub)
    kw = {"l2_form": "folded"} if form == "folded" else {}
    C = torch.from_numpy(sample_codebook(X, SD, dsub, rng))
    typed, twin, codes, _ = build_pair(_hasher(SD), dev(X), dsub, metric=metric, keys=corpus_keys, codebook=C, compat=False, **kw)
    assert_is_the_twin(typed, twin)
    P = keys.shape[1]
    deny = np.arange(0, typed.gid.shape[0], 3)
    ft, fw = typed.row_filter(deny=deny.tolist()), twin.row_filter(deny=deny.tolist())
    typed.window_rows = twin.window_rows = 0
    ra = typed.scan_tensors(q, keys, nkeys, k=10, want_keys=True)
    nq, nrows = _task_table(typed, SQ, P, 10, SD)
    d4 = (SD + 3) // 4
    shapes, single = set(), {True: set(), False: set()}
    for a, r in zip(nq.tolist(), nrows.tolist()):
        per_wave = {max(0, min(4, (a - wave + 3) // 4)) for wave in range(4)}
        shapes |= {(n, (r + 63) // 64) for n in per_wave}
        if r <= 64:
            single[r * d4 <= 1024] |= per_wave
    assert shapes == {(n, t) for n in range(5) for t in range(1, 5)}, sorted(shapes)
    assert single[True] == set(range(5)) and single[False] == set(range(5)), single
    assert {40, 41} <= set(nrows.tolist())                                      # both sides of the single-stage threshold
    rb = twin.scan_tensors(q, keys, nkeys, k=10, want_keys=True)
    assert_same_results(ra, rb, (form, "window 0"))
    _same(ra[3], rb[3], "keys64")
    for window, ks in ((0, (1, 10, 64, 65, 256)), (64, (1, 10, 64, 65, 256)), (128, (10, 65)), (256, (10, 256))):
        typed.window_rows = twin.window_rows = window
        for k in ks:
            for filt in (None, (ft, fw)):
                kt, kb = ({}, {}) if filt is None else ({"filter": filt[0]}, {"filter": filt[1]})
                ra, rb = typed.scan_tensors(q, keys, nkeys, k=k, want_keys=True, **kt), twin.scan_tensors(q, keys, nkeys, k=k, want_keys=True, **kb)
                assert typed.last_window == window and twin.last_window == window
                assert_same_results(ra, rb, (form, window, k, filt is not None))
                _same(ra[3], rb[3], ("keys64", form, window, k, filt is not None))
                assert typed.last_status.cpu().tolist() == twin.last_status.cpu().tolist()
        if window:
            assert int(typed.last_status.cpu()[0]) < len(nq)                    # fewer tasks than buckets: windows were shared
    denied = set(deny.tolist())
    assert not (set(ra[1].cpu().numpy().reshape(-1).tolist()) & denied)          # (the last call was filtered: no denied id came back)


def test_mass_ties_all_codes_equal():
    """Every row holds the same code bytes: every distance of a query is one value and the (distance, id) order decides every list."""
    from nlsh_amd.indexer import Indexer
    d, dsub, N, Q = 100, 8, 3000, 32
    rng = np.random.default_rng(3)
    C = torch.from_numpy(sample_codebook(real_rows(500, d, rng), d, dsub, rng))
    codes = torch.full((N, pq_ref.n_sub(d, dsub)), 37, dtype=torch.uint8)
    keys = dev(rng.integers(0, 6, size=N).astype(np.int32))
    qk, nk = dev(np.tile(np.arange(6, dtype=np.int32), (Q, 1))), dev(np.full(Q, 6, np.int32))
    q = dev(real_rows(Q, d, rng, special=False))
    for metric in ("l2", "cosine"):
        typed = Indexer(_hasher(d), codes.cuda(), _dist(metric), storage="pq", pq_dsub=dsub, pq_dim=d, quantiser=C, corpus_keys=keys, compat=False)
        twin = Indexer(_hasher(d), cpu_decode(codes, C, d).cuda(), _dist(metric), algo="tiled", corpus_keys=keys, compat=False)
        for k in (1, 64, 65, 256):
            ra, rb = typed.scan_tensors(q, qk, nk, k=k, want_keys=True), twin.scan_tensors(q, qk, nk, k=k, want_keys=True)
            assert_same_results(ra, rb, (metric, k))
            _same(ra[3], rb[3], "keys64")
        assert ra[1][:, :256].cpu().tolist() == [list(range(256))] * Q           # N rows at one distance: the 256 lowest ids, ascending


def test_facade_results_equal_the_twins():
    """`query()` lists and counts (compat on and off), `query_tensors`, ranked probes with a candidate budget, hash_times = 70 (the sliced
    scan), `query_with_keys` and a filter; the pq index always takes the two-step route."""
    d, dsub, N, Q, k = 32, 8, 6000, 256, 10
    rng = np.random.default_rng(21)
    X = real_rows(N, d, rng)
    q = dev(real_rows(Q, d, rng, special=False))
    C = torch.from_numpy(sample_codebook(X, d, dsub, rng))
    for compat in (True, False):
        hashing = _hasher(d, H=10, compat=compat)
        typed, twin, _, _ = build_pair(hashing, dev(X), dsub, codebook=C, compat=compat)
        assert_is_the_twin(typed, twin, cells=(64,))
        for kw in ({"hash_times": 1}, {"hash_times": 6}, {"hash_times": 70}, {"hash_times": 8, "probes": "ranked"},
                   {"hash_times": 16, "probes": "ranked", "candidate_budget": 40}):
            seed = {} if "probes" in kw else {"seed": 17}
            got = typed.query(q, k=k, **kw, **seed)
            assert typed.last_query_path == "two_step"
            want = twin.query(q, k=k, **kw, **seed)
            assert got[1] == want[1] and got[0] == want[0], kw
            assert_same_results(typed.query_tensors(q, k=k, **kw, **seed), twin.query_tensors(q, k=k, **kw, **seed), kw)
            assert typed.last_query_path == "two_step"
        allow = list(range(0, N, 2))
        assert_same_results(typed.query_tensors(q, k=k, hash_times=6, seed=2, filter=typed.row_filter(allow=allow)),
                            twin.query_tensors(q, k=k, hash_times=6, seed=2, filter=twin.row_filter(allow=allow)), "filter")
        key_lists = [[int(v) for v in typed._uniq_host[(7 * i) % typed.n_buckets:][:1 + i % 5]] + ([123456] if i % 9 == 0 else []) for i in range(Q)]
        got, want = typed.query_with_keys(q, key_lists, k=k), twin.query_with_keys(q, key_lists, k=k)
        assert got[0] == want[0] and got[1] == want[1]
        _same(got[2], want[2], "query_with_keys dist")
        _same(got[3], want[3], "query_with_keys idx")


# ---------------------------------------------------------------------------------------------- 4. mutation
class World:
    """A pq index, its float32 twin and the model of the codes they should hold (local order), mutated side by side: the pq index gets
    float32 rows or codes, the twin the CPU-decoded rows."""

    def __init__(self, metric, d, dsub, n, seed):
        from nlsh_amd.indexer import Indexer
        self.metric, self.d, self.dsub = metric, d, dsub
        self.rng = np.random.default_rng(seed)
        self.hashing = _hasher(d, H=8)
        X = real_rows(n, d, self.rng)
        self.C = sample_codebook(X, d, dsub, self.rng)
        self.typed = Indexer(self.hashing, dev(X), _dist(metric), storage="pq", pq_dsub=dsub, quantiser=torch.from_numpy(self.C), compat=False)
        self.codes = torch.from_numpy(pq_ref.pq_encode(X, self.C, d)[0])
        self.ids = np.arange(n, dtype=np.int32)
        self.twin = Indexer(self.hashing, self.decoded(self.codes).cuda(), _dist(metric), algo="tiled", compat=False)
        self.keys = self.typed.corpus_keys.cpu().numpy()
        self.q = dev(real_rows(64, d, self.rng, special=False))

    def decoded(self, codes):
        return cpu_decode(codes, self.C, self.d)

    def rows(self, n):
        X = real_rows(n, self.d, self.rng, special=False)
        return X, torch.from_numpy(pq_ref.pq_encode(X, self.C, self.d)[0])

    def add(self, n, as_float32, given_keys):
        X, codes = self.rows(n)
        keys = dev(self.rng.choice(self.keys, size=n).astype(np.int32)) if given_keys and len(self.keys) else None
        ids = self.typed.add(dev(X) if as_float32 else codes.cuda(), keys=keys)
        assert torch.equal(ids, self.twin.add(self.decoded(codes).cuda(), keys=keys))
        self.codes = torch.cat([self.codes, codes])
        self.ids = np.r_[self.ids, ids.cpu().numpy()].astype(np.int32)
        self.keys = self.typed.corpus_keys.cpu().numpy()

    def remove(self, ids):
        ids = np.asarray(ids, np.int64)
        n = self.typed.remove(ids.tolist())
        assert n == self.twin.remove(ids.tolist()) == int(np.isin(self.ids, ids).sum())
        stay = ~np.isin(self.ids, ids)
        self.codes, self.ids = self.codes[torch.from_numpy(stay)], self.ids[stay]
        self.keys = self.typed.corpus_keys.cpu().numpy()

    def update(self, n_add, ids_remove):
        X, codes = self.rows(n_add)
        ids_remove = np.asarray(ids_remove, np.int64)
        a = self.typed.update(add=dev(X), remove=ids_remove.tolist())
        b = self.twin.update(add=self.decoded(codes).cuda(), remove=ids_remove.tolist())
        assert torch.equal(a[0], b[0]) and a[1] == b[1]
        stay = ~np.isin(self.ids, ids_remove)
        self.codes = torch.cat([self.codes[torch.from_numpy(stay)], codes])
        self.ids = np.r_[self.ids[stay], a[0].cpu().numpy()].astype(np.int32)
        self.keys = self.typed.corpus_keys.cpu().numpy()

    def check(self):
        from nlsh_amd.indexer import Indexer
        assert len(self.keys) == len(self.ids) == len(self.codes)
        rebuilt = Indexer(self.hashing, self.codes.cuda(), _dist(self.metric), storage="pq", pq_dsub=self.dsub, pq_dim=self.d, compat=False,
                          corpus_keys=dev(self.keys), row_ids=dev(self.ids), quantiser=torch.from_numpy(self.C))
        for name in INDEX_ARRAYS + ("corpus_sorted",):
            _same(getattr(self.typed, name), getattr(rebuilt, name), ("rebuild", name))
        _same(self.typed.bucket_order[:self.typed.n_buckets], rebuilt.bucket_order[:rebuilt.n_buckets], "bucket_order")
        _same(self.typed.codebook.cpu(), torch.from_numpy(self.C), "the codebook is the index's for life")
        assert_is_the_twin(self.typed, self.twin, cells=(64,))
        if len(self.ids):
            assert_same_results(self.typed.query_tensors(self.q, k=5, hash_times=4, seed=5), self.twin.query_tensors(self.q, k=5, hash_times=4, seed=5),
                                "after mutation")


@pytest.mark.parametrize("metric, d, dsub", [("l2", 100, 8), ("cosine", 100, 16), ("l2", 12, 8), ("cosine", 16, 4)])
def test_mutations_equal_the_pq_rebuild_and_the_mutated_twin(metric, d, dsub):
    w = World(metric, d=d, dsub=dsub, n=4000, seed=len(metric) + d)
    w.check()
    w.add(300, as_float32=True, given_keys=False)
    w.check()
    w.remove(w.rng.choice(w.ids, size=500, replace=False))
    w.check()
    w.update(257, w.rng.choice(w.ids, size=100, replace=False))
    w.check()
    w.add(65, as_float32=False, given_keys=True)
    w.remove(np.r_[w.rng.choice(w.ids, size=123, replace=False), [10 ** 8]])
    w.check()
    assert w.typed.generation == 5
    bad = real_rows(5, d, w.rng, special=False)
    bad[3, d - 1] = np.nan
    with pytest.raises(ValueError, match=r"added row 3 holds a NaN or an infinity.*storage='pq'"):
        w.typed.add(dev(bad))
    with pytest.raises(ValueError, match=r"added rows must be float32 or uint8 \(codes\)"):
        w.typed.add(dev(bad).double())
    assert w.typed.generation == 5
    w.check()
    w.remove(w.ids.copy())                                            # emptied, then refilled with codes
    assert w.typed.n_buckets == 0 and w.typed.corpus_sorted.shape == (0, w.typed.row_stride)
    w.add(65, as_float32=False, given_keys=False)
    w.check()


# ---------------------------------------------------------------------------------------------- 5. refine
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_refine_on_a_pq_index_rescores_on_the_original_rows(metric):
    """Lists and distance bits of a refined pq index == the float32 scan's bits on the ORIGINAL rows (tests/refine_ref.py), re-ranked
    from the pq index's own stage-one candidates."""
    from nlsh_amd.indexer import Indexer
    from test_gpu_refine import D_F, H_F, N_F, _facade_world, assert_refined
    from test_gpu_refine import _hasher as refine_hasher
    w = _facade_world("sq8", metric)                                   # real-valued rows, the pair table over the originals
    hashing = refine_hasher(D_F, H=H_F, seed=77, mean=w["mean"], spread=w["spread"])
    ix = Indexer(hashing, dev(w["rows"]), _dist(metric), compat=False, storage="pq", pq_dsub=8, refine="device")
    assert ix.refine_store.n_rows == N_F and ix.refine_store.where == "device"
    q = dev(w["queries"])
    deny = ix.row_filter(deny=list(range(0, N_F, 3)))
    changed = 0
    for name, kw in (("sampled", dict(hash_times=10, seed=3)), ("ranked", dict(hash_times=10, probes="ranked")),
                     ("budget", dict(hash_times=16, probes="ranked", candidate_budget=300)), ("filter", dict(hash_times=10, seed=3, filter=deny))):
        for k in (1, 10, 64):
            i1, ri = assert_refined(ix, q, w["bits"], k, (metric, name, k), **kw)
            changed += int((ri != i1[:, :k]).any())
    assert changed, "a lossy storage whose stage-one order is never corrected tests nothing"
    # codes given: the store keeps what they decode to
    codes = stored_codes(ix)
    from_codes = Indexer(hashing, codes.cuda(), _dist(metric), compat=False, storage="pq", pq_dsub=8, pq_dim=D_F, quantiser=ix.codebook, refine="device")
    R = cpu_decode(codes, ix.codebook.cpu(), D_F)
    assert from_codes.refine_store.n_rows == N_F
    _same(from_codes.refine_store.rows[:N_F, :D_F].cpu().contiguous(), R, "store of decoded rows")


# ---------------------------------------------------------------------------------------------- 6. multi-table
def test_multi_table_shares_one_codebook_and_is_the_merge_of_its_tables_twins():
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.multitable import MultiTableIndexer
    d, dsub, N, Q, T = 20, 8, 4000, 128, 2
    rng = np.random.default_rng(6)
    X = real_rows(N, d, rng)
    q = dev(real_rows(Q, d, rng, special=False))
    hashings = [make_hashing(d, (32,), 9, *synth.make_weights([d, 32, 9], seed=50 + t), compat=False) for t in range(T)]
    mt = MultiTableIndexer(hashings, dev(X), _dist("l2"), storage="pq", pq_dsub=dsub)
    assert mt.storage == "pq" and len(mt.tables) == T
    C = mt.tables[0].codebook
    _same(mt.tables[1].codebook, C, "one codebook for all tables")
    codes = stored_codes(mt.tables[0])
    assert torch.equal(codes, stored_codes(mt.tables[1]))
    R = cpu_decode(codes, C.cpu(), d)
    twins = [Indexer(h, R.cuda(), _dist("l2"), algo="tiled", compat=False) for h in hashings]
    for a, b in zip(mt.tables, twins):
        assert_is_the_twin(a, b, cells=(64,))
    for k in (10, 100):
        for kw in (dict(hash_times=6, probes="ranked"), dict(hash_times=12, probes="ranked", candidate_budget=150)):
            per = [t.query_tensors(q, k=k, want_keys=True, **kw) for t in twins]
            keys_all = np.stack([p[3].cpu().numpy().view(np.uint64) for p in per])
            want_dist, want_idx, want_keys = MT.unique_merge_reference(keys_all, k)
            dist, idx, ncand, keys = mt.query_tensors(q, k=k, want_keys=True, **kw)
            assert np.array_equal(keys.cpu().numpy().view(np.uint64), want_keys), (k, kw)
            assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(dist.cpu().numpy().view(np.uint32), want_dist.view(np.uint32))
            assert np.array_equal(ncand.cpu().numpy(), np.stack([p[2].cpu().numpy() for p in per]).sum(0, dtype=np.int64).astype(np.int32))
    more = real_rows(100, d, rng, special=False)
    ids = mt.add(dev(more))
    Rm = cpu_decode(pq_ref.pq_encode(more, C.cpu().numpy(), d)[0], C.cpu(), d)
    for a, b in zip(mt.tables, twins):
        assert torch.equal(ids, b.add(Rm.cuda()))
        assert_is_the_twin(a, b, cells=(64,))


# ---------------------------------------------------------------------------------------------- 7. the derived bound
def test_l2_distances_stay_within_the_quantisation_error_of_the_original_rows():
    """The first of the two tests with a tolerance, and the tolerance is derived: a pq L2 distance is the distance to x^ = decode(encode(x)),
    so by the triangle inequality it differs from the distance to the ORIGINAL row x by at most ||x - x^||_2 (float64, per returned pair)
    -- plus the float32-accumulation allowance of the sq8 bound test, 2e-5 * max(1, distance).  Every returned (query, row) is held to it."""
    from nlsh_amd.indexer import Indexer
    N, d, dsub, Q, k = 20000, 32, 8, 256, 10
    rng = np.random.default_rng(77)
    scale = rng.uniform(0.05, 4.0, size=d)
    X = (rng.standard_normal((N, d)) * scale + rng.uniform(-2, 2, size=d) * scale).astype(np.float32)
    qv = (rng.standard_normal((Q, d)) * scale).astype(np.float32)
    ix = Indexer(_hasher(d, H=8), dev(X), _dist("l2"), storage="pq", pq_dsub=dsub, compat=False)
    dist, idx = ix.query_tensors(dev(qv), k=k, hash_times=8, seed=4)[:2]
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    found = idx >= 0
    assert found.sum() > Q * k // 2
    qi = np.nonzero(found)[0]
    rows = idx[found]
    Xh = cpu_decode(stored_codes(ix), ix.codebook.cpu(), d).numpy().astype(np.float64)
    eps = np.float64(np.float32(1e-6))
    exact = np.sqrt((((qv[qi].astype(np.float64) - X[rows].astype(np.float64)) + eps) ** 2).sum(1))
    qerr = np.sqrt(((X[rows].astype(np.float64) - Xh[rows]) ** 2).sum(1))
    err = np.abs(dist[found].astype(np.float64) - exact)
    bound = qerr + 2e-5 * np.maximum(1.0, exact)
    print(f"pq distance error: max {err.max():.5f}, mean quantisation error {qerr.mean():.5f}, max ratio {(err / bound).max():.3f}")
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------- 8. training
def test_pq_train_is_seeded_and_lowers_the_quantisation_error():
    from nlsh_amd.training import pq_train
    d, dsub, n = 20, 8, 6000
    rng = np.random.default_rng(12)
    centres = rng.standard_normal((8, d)) * 20.0                       # 8 well-separated Gaussian blobs
    X = (centres[rng.integers(0, 8, n)] + rng.standard_normal((n, d))).astype(np.float32)
    M = pq_ref.n_sub(d, dsub)

    def mse(cb):
        C = cb.cpu().numpy()
        R = pq_ref.pq_decode(pq_ref.pq_encode(X, C, d)[0], C, d)
        return float(((X.astype(np.float64) - R) ** 2).sum(1).mean())

    cb0 = pq_train(dev(X), dsub, iters=0, seed=3)
    cb = pq_train(dev(X), dsub, iters=10, seed=3)
    for c in (cb0, cb):
        assert tuple(c.shape) == (M, 256, dsub) and c.dtype == torch.float32 and c.is_cuda and bool(torch.isfinite(c).all())
        assert bool((c[M - 1, :, d - (M - 1) * dsub:] == 0).all()), "tail columns are zero"
    _same(pq_train(dev(X), dsub, iters=10, seed=3), cb, "same seed, same codebook")
    assert not torch.equal(pq_train(dev(X), dsub, iters=10, seed=4), cb)
    e0, e10 = mse(cb0), mse(cb)
    print(f"pq_train: mean squared quantisation error {e0:.4f} at 0 iterations, {e10:.4f} after 10")
    assert e10 <= (1 + 1e-4) * e0
    # fewer than 256 sample rows: the rows repeat; a sample smaller than the corpus; non-finite rows are left out
    small = pq_train(dev(X[:100]), dsub, iters=2, seed=0)
    assert tuple(small.shape) == (M, 256, dsub) and bool(torch.isfinite(small).all())
    Y = X.copy()
    Y[5, 3] = np.nan
    assert bool(torch.isfinite(pq_train(dev(Y), 4, iters=1, seed=0, sample=512)).all())
