"""sq8 corpus storage against ITS DEFINITION: with S the stored codes and R = deq(S), `Indexer(hashing, corpus, dist, storage="sq8")` is,
word for word, the float32 index over R -- every index array, every distance bit, id, candidate count and result list.  The reference
is always the existing float32 path (`algo="tiled"` forced on the twin) on R with the same `corpus_keys=`, never the code under test;
the quantiser and the codes are held against the rule evaluated by torch on the CPU (tests/test_sq8_storage_cpu.py restates it in
numpy).  Every comparison but the last test's is `torch.equal` on raw bits: no tolerance."""
import numpy as np
import pytest
import torch

from helpers import dev, make_hashing
from helpers import task_table as _task_table
from nlsh_amd import _capi, synth
from test_gpu_corpus_storage import GROUPS, INDEX_ARRAYS, SD, SIZES, SQ, TINY, _dist, _same, assert_same_results
from test_sq8_storage_cpu import sq8_decode, sq8_encode, sq8_train

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- the rule, by torch on the CPU
def rule_train(x):
    x = x.float()
    lo, hi = x.min(dim=0).values + 0.0, x.max(dim=0).values + 0.0
    return lo, torch.where(hi == lo, torch.ones_like(lo), (hi - lo) / 255.0)


def rule_encode(x, lo, step):
    t = ((x.float() - lo) / step).round()
    return t.clamp(0, 255).to(torch.uint8), ((t < 0) | (t > 255)).any(dim=1)


def rule_decode(codes, lo, step):
    return codes.float() * step + lo


def _hasher(d, H=16, compat=False):
    Ws, bs = synth.make_weights([d, 32, H], seed=d)
    return make_hashing(d, (32,), H, Ws, bs, compat=compat)


def real_rows(n, d, rng, special=True):
    """[n, d] float32: Gaussian with per-dimension scales and offsets.  special: column 0 constant, column 1 (d >= 2) holds both signed
    zeros as its minimum, column 2 (d >= 3) spans [0, 510] on integers -- step 2 exactly, so the odd values lie on .5 code boundaries."""
    X = (rng.standard_normal((n, d)) * rng.uniform(0.05, 8.0, size=d) + rng.uniform(-4.0, 4.0, size=d)).astype(np.float32)
    if special:
        X[:, 0] = np.float32(-1.75)
        if d >= 2:
            X[:, 1] = np.abs(X[:, 1])
            X[::3, 1], X[1::7, 1] = np.float32(-0.0), np.float32(0.0)
        if d >= 3:
            X[:, 2] = rng.integers(0, 511, size=n).astype(np.float32)
            X[:6, 2] = [0, 510, 1, 3, 5, 509]
    return X


def views_of(X, dtype):
    """The rows as contiguous, row-strided and misaligned device tensors of `dtype`."""
    n, d = X.shape
    t = dev(X).to(dtype)
    wide = torch.zeros((n, d + 8 + 3), dtype=dtype, device="cuda")
    wide[:, 1:d + 1] = t
    aligned = torch.zeros((n, (d + 15) // 16 * 16 + 16), dtype=dtype, device="cuda")
    aligned[:, :d] = t
    return {"contiguous": t, "row-strided": aligned[:, :d], "misaligned": wide[:, 1:d + 1]}


def _raw_bits(t):
    return t.contiguous().view(torch.int32)


def assert_is_the_twin(typed, twin, cells=(64, 256)):
    """Every array the definition names; `corpus_sorted` holds the codes, whose decode is the twin's sorted copy."""
    d = typed.dim
    assert typed.storage == "sq8" and typed.corpus_sorted.dtype == torch.uint8 and twin.corpus_sorted.dtype == torch.float32
    assert typed.row_stride % 16 == 0 and typed.row_stride >= d
    assert typed.row_stride == twin.row_stride and typed.n_buckets == twin.n_buckets
    for name in INDEX_ARRAYS:
        _same(getattr(typed, name), getattr(twin, name), name)
    _same(typed.bucket_order[:typed.n_buckets], twin.bucket_order[:twin.n_buckets], "bucket_order")
    lo, step = typed.quantiser
    assert lo.shape == (d,) and step.shape == (d,) and lo.dtype == step.dtype == torch.float32 and lo.is_cuda and step.is_cuda
    _same(typed._dequantised(typed.corpus_sorted[:, :d]), twin.corpus_sorted[:, :d].contiguous(), "deq(corpus_sorted)")
    assert not bool((typed.corpus_sorted[:, d:] != 0).any()), "padding columns are stored as code 0"
    assert not bool((twin.corpus_sorted[:, d:] != 0).any())
    assert bool((typed._qlo[d:] == 0).all()) and bool((typed._qstep[d:] == 1).all()), "the quantiser is padded to the pitch with lo = 0, step = 1"
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


def build_pair(hashing, source, metric="l2", row_align=4, keys=None, quantiser=None, **kw):
    """(sq8 index built from `source`, its float32 twin built from R = deq(stored codes)), same keys, the twin on the tiled schedule with
    the sq8 pitch.  R is computed by torch ON THE CPU from the codes the index stored, un-permuted."""
    from nlsh_amd.indexer import Indexer
    ck = None if keys is None else dev(np.asarray(keys, np.int32))
    typed = Indexer(hashing, source, _dist(metric), storage="sq8", row_align=row_align, corpus_keys=ck, quantiser=quantiser, **kw)
    lo, step = (t.cpu() for t in typed.quantiser)
    codes = torch.empty((typed.gid.shape[0], typed.dim), dtype=torch.uint8)
    codes[typed.perm.long().cpu()] = typed.corpus_sorted[:, :typed.dim].cpu()
    R = rule_decode(codes, lo, step)
    twin = Indexer(hashing, R.cuda(), _dist(metric), algo="tiled", row_align=max(row_align, 16), corpus_keys=ck, **kw)
    return typed, twin, codes, R


# ---------------------------------------------------------------------------------------------- quantiser and codes
@pytest.mark.parametrize("d", [1, 3, 4, 7, 16, 17, 100, 260, 1024])
def test_quantiser_and_codes_equal_the_rule(d):
    from nlsh_amd.indexer import Indexer
    N = 777
    rng = np.random.default_rng(d)
    X = real_rows(N, d, rng)
    keys = dev(rng.integers(-6, 7, size=N).astype(np.int32))
    hashing = _hasher(d)
    for dtype in (torch.float32, torch.float16):
        Xs = torch.from_numpy(X).to(dtype)                                      # the rows as the source holds them
        lo, step = rule_train(Xs)
        codes, clamped = rule_encode(Xs, lo, step)
        assert not bool(clamped.any())
        if dtype == torch.float32:                                              # ... and the numpy restatement says the same
            nlo, nstep = sq8_train(X)
            assert np.array_equal(nlo.view(np.int32), lo.numpy().view(np.int32)) and np.array_equal(nstep.view(np.int32), step.numpy().view(np.int32))
            assert np.array_equal(sq8_encode(X, nlo, nstep)[0], codes.numpy())
            assert np.array_equal(sq8_decode(codes.numpy(), nlo, nstep).view(np.int32), rule_decode(codes, lo, step).numpy().view(np.int32))
        if d >= 3:
            assert float(step[0]) == 1.0 and float(step[2]) == 2.0 and lo[1].view(torch.int32).item() == 0      # constant, .5 ties, +0
            assert codes[:6, 2].tolist() == [0, 255, 0, 2, 2, 254]                                               # ties go to even
        for name, src in views_of(X, dtype).items():
            for metric in ("l2", "cosine"):
                ix = Indexer(hashing, src, _dist(metric), storage="sq8", corpus_keys=keys, row_align=4 if metric == "l2" else 32)
                what = (d, dtype, name, metric)
                glo, gstep = ix.quantiser
                _same(glo.cpu(), lo, (what, "lo"))
                _same(gstep.cpu(), step, (what, "step"))
                assert torch.equal(ix.corpus_sorted[:, :d].cpu(), codes[ix.perm.long().cpu()]), (what, "codes")
                assert not bool((ix.corpus_sorted[:, d:] != 0).any()) and ix.last_clamped_rows == 0, what
                _same(ix._dequantised(ix.corpus_sorted[:, :d]).cpu(), rule_decode(codes, lo, step)[ix.perm.long().cpu()], (what, "decode"))
    # a given quantiser narrower than the data: finite values saturate at both ends and the rows are counted
    lo = torch.from_numpy(np.quantile(X, 0.2, axis=0).astype(np.float32))
    step = torch.from_numpy(((np.quantile(X, 0.8, axis=0) - lo.numpy()) / 255 + 1e-3).astype(np.float32))
    codes, clamped = rule_encode(torch.from_numpy(X), lo, step)
    ix = Indexer(hashing, dev(X), _dist("l2"), storage="sq8", corpus_keys=keys, quantiser=(lo, step))
    assert torch.equal(ix.corpus_sorted[:, :d].cpu(), codes[ix.perm.long().cpu()])
    assert ix.last_clamped_rows == int(clamped.sum()) and (d == 1 or ix.last_clamped_rows > 0)
    if d > 1:
        assert int(codes.min()) == 0 and int(codes.max()) == 255
    _same(ix.quantiser[0].cpu(), lo, "given lo")
    _same(ix.quantiser[1].cpu(), step, "given step")


def test_training_through_the_c_abi_overflow_and_empty():
    """`nlsh_sq8_train` itself: more rows than one workgroup sweep, a column whose range overflows (step = +inf, refused by the facade), no
    rows at all (the identity), and the smallest non-finite row reported."""
    from nlsh_amd.indexer import Indexer
    L, d, stride = _capi.lib(), 5, 16
    rng = np.random.default_rng(3)
    X = real_rows(70000, d, rng)

    def train(rows):
        n = rows.shape[0]
        lo = torch.full((stride,), 7.0, device="cuda")
        step = torch.full((stride,), 7.0, device="cuda")
        bad = torch.zeros((1,), dtype=torch.int32, device="cuda")
        wb = L.nlsh_sq8_train_workspace(n, d)
        ws = torch.empty((max(wb, 16),), dtype=torch.uint8, device="cuda")
        _capi.check(L.nlsh_sq8_train(_capi.ptr(rows), _capi.STORE_F32, rows.stride(0) if n else d, d, n, _capi.ptr(lo), _capi.ptr(step), stride,
                                     _capi.ptr(bad), _capi.ptr(ws), wb, torch.cuda.current_stream().cuda_stream))
        return lo.cpu(), step.cpu(), int(bad.item())

    lo, step, bad = train(dev(X))
    rlo, rstep = rule_train(torch.from_numpy(X))
    assert bad == -1
    _same(lo[:d], rlo, "lo")
    _same(step[:d], rstep, "step")
    assert lo[d:].tolist() == [0.0] * (stride - d) and step[d:].tolist() == [1.0] * (stride - d)
    lo, step, bad = train(torch.empty((0, d), device="cuda"))
    assert bad == -1 and lo.tolist() == [0.0] * stride and step.tolist() == [1.0] * stride
    Y = X[:3000].copy()
    Y[5, 3], Y[9, 3] = np.float32(3e38), np.float32(-3e38)
    lo, step, bad = train(dev(Y))
    assert bad == -1 and np.isinf(float(step[3])) and np.isfinite(step[:3].numpy()).all()
    with pytest.raises(ValueError, match="corpus column 3"):
        Indexer(_hasher(d), dev(Y), _dist("l2"), storage="sq8", corpus_keys=dev(np.zeros(3000, np.int32)))
    Y = X[:3000].copy()
    Y[2222, 1], Y[77, 4], Y[2999, 0] = np.nan, np.inf, -np.inf
    assert train(dev(Y))[2] == 77


# ---------------------------------------------------------------------------------------------- index arrays
@pytest.mark.parametrize("d", [1, 3, 4, 7, 16, 17, 100, 260, 1024])
def test_index_arrays_equal_the_float32_twins(d):
    """l2 at the default pitch and cosine (the inv_norm bits) at row_align=32, keys given and keys from the hash of the decoded rows; one
    query batch through each pair.  float32 and float16 sources, and the codes themselves with the quantiser."""
    from nlsh_amd.indexer import Indexer
    N, Q = 2000, 64
    rng = np.random.default_rng(100 + d)
    X = real_rows(N, d, rng)
    hashing = _hasher(d)
    q = dev(real_rows(Q, d, rng, special=False))
    pool = np.unique(np.r_[hashing.hash_device(q, n=1)[0].reshape(-1).cpu().numpy(), np.arange(100, 104)]).astype(np.int32)
    given = rng.choice(pool, size=N).astype(np.int32)
    for metric, row_align in (("l2", 4), ("cosine", 32)):
        for keys in (given, None):
            for src in (dev(X), dev(X).half()):
                typed, twin, codes, R = build_pair(hashing, src, metric=metric, row_align=row_align, keys=keys)
                assert typed.row_stride == (d + 15) // 16 * 16 if row_align == 4 else typed.row_stride % 32 == 0
                assert_is_the_twin(typed, twin)
                ra = typed.query_tensors(q, k=10, hash_times=4, seed=3)
                assert typed.last_query_path == "two_step" and typed.last_algo == _capi.SCAN_BUCKET_TILED
                assert_same_results(ra, twin.query_tensors(q, k=10, hash_times=4, seed=3), (metric, row_align, keys is None, src.dtype))
                if keys is not None:
                    assert int(ra[2].sum()) > 0
        # a uint8 corpus is codes: with the quantiser it is the same index
        again = Indexer(hashing, codes.cuda(), _dist(metric), storage="sq8", row_align=row_align, corpus_keys=dev(given), quantiser=typed.quantiser)
        ref = Indexer(hashing, R.cuda(), _dist(metric), algo="tiled", row_align=max(row_align, 16), corpus_keys=dev(given))
        assert_is_the_twin(again, ref, cells=(64,))


def test_keys_come_from_the_decoded_rows_and_the_chunked_encode():
    """N > HASH_BATCH: the keys are those of R = deq(enc(X)), hashed HASH_BATCH rows at a time, not of the caller's rows."""
    from nlsh_amd.indexer import HASH_BATCH, Indexer
    d, N = 24, HASH_BATCH + 904
    rng = np.random.default_rng(5)
    X = real_rows(N, d, rng)
    hashing = _hasher(d)
    typed, twin, _, R = build_pair(hashing, dev(X), metric="l2")
    assert_is_the_twin(typed, twin, cells=(64,))
    unrounded = Indexer(hashing, dev(X), _dist("l2"), algo="tiled")
    assert not torch.equal(unrounded.corpus_keys, typed.corpus_keys)            # (the quantisation really moves some keys: the test can tell)


# ---------------------------------------------------------------------------------------------- the identity quantiser
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_identity_quantiser_is_the_uint8_index(metric):
    from nlsh_amd.indexer import Indexer
    d, N, Q = 100, 3000, 64
    rng = np.random.default_rng(8)
    S = rng.integers(0, 256, size=(N, d)).astype(np.uint8)
    S[0], S[1] = 0, 255
    keys = dev(rng.integers(0, 40, size=N).astype(np.int32))
    qk = dev(np.stack([rng.choice(40, size=6, replace=False) for _ in range(Q)]).astype(np.int32))      # a row's keys are distinct
    nk = dev(np.full(Q, 6, np.int32))
    q = dev(rng.integers(0, 256, size=(Q, d)).astype(np.float32) + rng.standard_normal((Q, d)).astype(np.float32) * 0.25)
    hashing = _hasher(d)
    ident = (torch.zeros(d), torch.ones(d))
    u8 = Indexer(hashing, dev(S), _dist(metric), storage="uint8", corpus_keys=keys, compat=False)
    for src in (dev(S), dev(S).float(), dev(S).half()):
        sq = Indexer(hashing, src, _dist(metric), storage="sq8", corpus_keys=keys, quantiser=ident, compat=False)
        assert sq.last_clamped_rows == 0
        for name in INDEX_ARRAYS + ("corpus_sorted",):
            _same(getattr(sq, name), getattr(u8, name), (name, src.dtype))
        for k in (1, 10, 100):
            assert_same_results(sq.scan_tensors(q, qk, nk, k=k), u8.scan_tensors(q, qk, nk, k=k), (k, src.dtype))


# ---------------------------------------------------------------------------------------------- scan across task shapes
def _shape_world(seed):
    """The bucket world of tests/test_gpu_corpus_storage.py (SIZES x GROUPS and a run of TINY buckets) over real-valued rows."""
    rng = np.random.default_rng(seed)
    buckets = [(s, m) for s in SIZES for m in GROUPS] + [(1 + i % 6, 1 + i % 3) for i in range(TINY)]
    N = sum(s for s, _ in buckets)
    X = real_rows(N, SD, rng)
    keys = np.repeat(np.arange(len(buckets), dtype=np.int32) * 3 - 200, [s for s, _ in buckets])
    order = rng.permutation(N)
    corpus_keys = np.empty(N, np.int32)
    corpus_keys[order] = keys
    first = {b: np.flatnonzero(corpus_keys == b * 3 - 200) for b in range(len(buckets))}
    ties = next(b for b, (s, m) in enumerate(buckets) if s == 256 and m == 17)
    X[first[ties]] = X[first[ties][0]]                              # a bucket of identical rows: the (distance, id) order decides
    key_lists = [[] for _ in range(SQ)]
    for b, (s, m) in enumerate(buckets):
        for qi in rng.choice(SQ, size=m, replace=False):
            key_lists[qi].append(int(b * 3 - 200))
    for qi in range(SQ):
        rng.shuffle(key_lists[qi])
    key_lists[7].insert(1, 999999)                                  # an unknown key
    P = max(len(ks) for ks in key_lists)
    assert P <= _capi.MAX_PROBES
    tab, cnt = np.zeros((SQ, P), np.int32), np.zeros((SQ,), np.int32)
    for qi, ks in enumerate(key_lists):
        tab[qi, :len(ks)], cnt[qi] = ks, len(ks)
    return X, corpus_keys, buckets, dev(tab), dev(cnt), dev(real_rows(SQ, SD, rng, special=False))


@pytest.mark.parametrize("form", ["l2", "folded", "cosine"])
def test_scan_equals_the_twin_on_every_task_shape(form):
    metric = "cosine" if form == "cosine" else "l2"
    X, corpus_keys, buckets, keys, nkeys, q = _shape_world(seed=11 + len(form))
    kw = {"l2_form": "folded"} if form == "folded" else {}
    typed, twin, _, _ = build_pair(_hasher(SD), dev(X), metric=metric, keys=corpus_keys, compat=False, **kw)
    assert_is_the_twin(typed, twin)
    P = keys.shape[1]
    deny = np.arange(0, typed.gid.shape[0], 3)                       # a third of the rows denied, the ties bucket's among them
    ft, fw = typed.row_filter(deny=deny.tolist()), twin.row_filter(deny=deny.tolist())
    # ---- window 0: one task list per bucket, so the task table provably holds every shape
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
    assert len(nq) == sum(((m + 15) // 16) * ((s + 255) // 256) for s, m in buckets)
    rb = twin.scan_tensors(q, keys, nkeys, k=10, want_keys=True)
    assert_same_results(ra, rb, (form, "window 0"))
    _same(ra[3], rb[3], "keys64")
    for window, ks in ((0, (1, 10, 64, 100, 256)), (64, (1, 10, 64, 100, 256)), (128, (10, 100)), (256, (10, 100))):
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
    ra = typed.scan_tensors(q, keys, nkeys, k=256)
    dist, idx = ra[0].cpu().numpy(), ra[1].cpu().numpy()
    for row_d, row_i in zip(dist, idx):                                           # the ties bucket: ids ascending within one distance
        same = (row_d[1:] == row_d[:-1]) & (row_i[1:] >= 0)
        assert np.all(row_i[1:][same] > row_i[:-1][same])


# ---------------------------------------------------------------------------------------------- facade
def test_facade_results_equal_the_twins():
    """`query()` lists and counts with the F7 short-list fallback (compat on and off), `query_tensors`, ranked probes, the candidate budget,
    hash_times > 64 (the sliced scan), `query_with_keys` and a filter; the sq8 index always takes the two-step route."""
    d, N, Q, k = 32, 6000, 512, 10
    rng = np.random.default_rng(21)
    X = real_rows(N, d, rng)
    X[N // 2:] = X[:N - N // 2]                                    # every row twice: distance ties across the corpus
    q = dev(real_rows(Q, d, rng, special=False))
    for compat in (True, False):
        hashing = _hasher(d, H=10, compat=compat)
        typed, twin, _, _ = build_pair(hashing, dev(X), metric="l2", compat=compat)
        assert_is_the_twin(typed, twin, cells=(64,))
        for kw in ({"hash_times": 1}, {"hash_times": 6}, {"hash_times": 80}, {"hash_times": 8, "probes": "ranked"},
                   {"hash_times": 16, "probes": "ranked", "candidate_budget": 40}):
            seed = {} if "probes" in kw else {"seed": 17}
            got = typed.query(q, k=k, **kw, **seed)
            assert typed.last_query_path == "two_step"
            want = twin.query(q, k=k, **kw, **seed)
            assert got[1] == want[1] and got[0] == want[0], kw
            if kw == {"hash_times": 1}:
                assert min(want[1]) < k <= max(want[1]), "both the short-list fallback (F7) and full lists are exercised"
            assert_same_results(typed.query_tensors(q, k=k, **kw, **seed), twin.query_tensors(q, k=k, **kw, **seed), kw)
            assert typed.last_query_path == "two_step"
        assert_same_results(typed.query_tensors(q, k=100, hash_times=6, seed=2), twin.query_tensors(q, k=100, hash_times=6, seed=2), "k = 100")
        allow = list(range(0, N, 2))
        assert_same_results(typed.query_tensors(q, k=k, hash_times=6, seed=2, filter=typed.row_filter(allow=allow)),
                            twin.query_tensors(q, k=k, hash_times=6, seed=2, filter=twin.row_filter(allow=allow)), "filter")
        key_lists = [[int(v) for v in typed._uniq_host[(7 * i) % typed.n_buckets:][:1 + i % 5]] + ([123456] if i % 9 == 0 else []) for i in range(Q)]
        got, want = typed.query_with_keys(q, key_lists, k=k), twin.query_with_keys(q, key_lists, k=k)
        assert got[0] == want[0] and got[1] == want[1]
        _same(got[2], want[2], "query_with_keys dist")
        _same(got[3], want[3], "query_with_keys idx")


def test_multi_table_shares_one_quantiser_and_equals_its_twin():
    from nlsh_amd.multitable import MultiTableIndexer
    d, N, Q, T = 20, 4000, 128, 3
    rng = np.random.default_rng(6)
    X = real_rows(N, d, rng)
    q = dev(real_rows(Q, d, rng, special=False))
    hashings = [make_hashing(d, (32,), 9, *synth.make_weights([d, 32, 9], seed=50 + t), compat=False) for t in range(T)]
    mt = MultiTableIndexer(hashings, dev(X), _dist("l2"), storage="sq8")
    assert mt.storage == "sq8" and len(mt.tables) == T
    lo, step = mt.tables[0].quantiser
    rlo, rstep = rule_train(torch.from_numpy(X))
    _same(lo.cpu(), rlo, "lo")
    _same(step.cpu(), rstep, "step")
    for t in mt.tables[1:]:
        _same(t.quantiser[0], lo, "one lo for all tables")
        _same(t.quantiser[1], step, "one step for all tables")
    R = rule_decode(rule_encode(torch.from_numpy(X), rlo, rstep)[0], rlo, rstep)
    twin = MultiTableIndexer(hashings, R.cuda(), _dist("l2"), row_align=16)
    for a, b in zip(mt.tables, twin.tables):
        assert_is_the_twin(a, b, cells=(64,))
    for kw in ({"hash_times": 4, "seed": 9}, {"hash_times": 6, "probes": "ranked"}):
        assert_same_results(mt.query_tensors(q, k=10, **kw), twin.query_tensors(q, k=10, **kw), kw)
        assert mt.query(q, k=10, **kw) == twin.query(q, k=10, **kw)
    # add forwards: every table encodes with the shared quantiser
    more = real_rows(100, d, rng, special=False)
    ids = mt.add(dev(more))
    Rm = rule_decode(rule_encode(torch.from_numpy(more), rlo, rstep)[0], rlo, rstep)
    assert torch.equal(ids, twin.add(Rm.cuda()))
    for a, b in zip(mt.tables, twin.tables):
        assert_is_the_twin(a, b, cells=(64,))
    assert_same_results(mt.query_tensors(q, k=10, hash_times=4, seed=9), twin.query_tensors(q, k=10, hash_times=4, seed=9), "after add")


# ---------------------------------------------------------------------------------------------- mutation
class World:
    """An sq8 index, its float32 twin and the model of the codes they should hold (local order), mutated side by side: the sq8 index
    gets float32 rows or codes, the twin the decoded rows (torch, CPU)."""

    def __init__(self, metric, d, n, seed):
        from nlsh_amd.indexer import Indexer
        self.metric, self.d = metric, d
        self.rng = np.random.default_rng(seed)
        self.hashing = _hasher(d, H=8)
        X = real_rows(n, d, self.rng)
        self.typed = Indexer(self.hashing, dev(X), _dist(metric), storage="sq8", compat=False)
        self.lo, self.step = (t.cpu() for t in self.typed.quantiser)
        self.codes = rule_encode(torch.from_numpy(X), self.lo, self.step)[0]
        self.ids = np.arange(n, dtype=np.int32)
        self.twin = Indexer(self.hashing, self.decoded(self.codes).cuda(), _dist(metric), algo="tiled", compat=False, row_align=16)
        self.keys = self.typed.corpus_keys.cpu().numpy()
        self.q = dev(real_rows(64, d, self.rng, special=False))

    def decoded(self, codes):
        return rule_decode(codes, self.lo, self.step)

    def rows(self, n):
        """New float rows inside the trained range (so nothing saturates) -> (float32 rows, their codes by the rule)."""
        lo, step = self.lo.numpy(), self.step.numpy()
        X = (lo + self.rng.uniform(0, 255, size=(n, self.d)) * step).astype(np.float32)
        codes, clamped = rule_encode(torch.from_numpy(X), self.lo, self.step)
        return X, codes, int(clamped.sum())

    def add(self, n, as_float32, given_keys):
        X, codes, n_clamped = self.rows(n)
        keys = dev(self.rng.choice(self.keys, size=n).astype(np.int32)) if given_keys and len(self.keys) else None
        ids = self.typed.add(dev(X) if as_float32 else codes.cuda(), keys=keys)
        assert self.typed.last_clamped_rows == (n_clamped if as_float32 else 0)
        ids2 = self.twin.add(self.decoded(codes).cuda(), keys=keys)
        assert torch.equal(ids, ids2)
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
        X, codes, _ = self.rows(n_add)
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
        rebuilt = Indexer(self.hashing, self.codes.cuda(), _dist(self.metric), storage="sq8", compat=False, corpus_keys=dev(self.keys),
                          row_ids=dev(self.ids), quantiser=(self.lo, self.step))
        for name in INDEX_ARRAYS + ("corpus_sorted",):
            _same(getattr(self.typed, name), getattr(rebuilt, name), ("rebuild", name))
        _same(self.typed.bucket_order[:self.typed.n_buckets], rebuilt.bucket_order[:rebuilt.n_buckets], "bucket_order")
        _same(self.typed.quantiser[0].cpu(), self.lo, "lo is the index's for life")
        _same(self.typed.quantiser[1].cpu(), self.step, "step is the index's for life")
        assert_is_the_twin(self.typed, self.twin, cells=(64,))
        if len(self.ids):
            assert_same_results(self.typed.query_tensors(self.q, k=5, hash_times=4, seed=5), self.twin.query_tensors(self.q, k=5, hash_times=4, seed=5),
                                "after mutation")


@pytest.mark.parametrize("d", [7, 100])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_mutations_equal_the_sq8_rebuild_and_the_mutated_twin(metric, d):
    w = World(metric, d=d, n=5000, seed=len(metric) + d)
    w.add(300, as_float32=True, given_keys=False)
    w.check()
    w.remove(w.rng.choice(w.ids, size=500, replace=False))
    w.check()
    w.update(257, w.rng.choice(w.ids, size=100, replace=False))
    w.check()
    w.add(65, as_float32=False, given_keys=True)
    w.remove(np.r_[w.rng.choice(w.ids, size=123, replace=False), [10 ** 8]])
    w.update(40, w.rng.choice(w.ids, size=77, replace=False))
    w.check()
    assert w.typed.generation == 6
    # a row outside the trained range saturates to codes 0 / 255 and is counted; the twin gets the saturated row
    lo, step = w.lo.numpy(), w.step.numpy()
    far = np.stack([lo - 1000 * step - 5, lo + 1000 * step + 5, lo + 10 * step]).astype(np.float32)
    ids = w.typed.add(dev(far))
    assert w.typed.last_clamped_rows == 2
    where = {int(g): p for p, g in enumerate(w.typed.gid.cpu().tolist())}
    stored = w.typed.corpus_sorted[[where[int(i)] for i in ids.cpu().tolist()]][:, :d].cpu()
    assert bool((stored[0] == 0).all()) and bool((stored[1] == 255).all()) and stored[2].tolist() == [10] * d
    w.twin.add(w.decoded(stored).cuda())
    w.codes, w.ids, w.keys = torch.cat([w.codes, stored]), np.r_[w.ids, ids.cpu().numpy()].astype(np.int32), w.typed.corpus_keys.cpu().numpy()
    w.check()


def test_an_emptied_index_is_refilled():
    w = World("cosine", d=7, n=300, seed=4)
    w.remove(w.ids.copy())
    assert w.typed.n_buckets == 0 and w.typed.corpus_sorted.shape == (0, w.typed.row_stride) and w.typed.corpus_sorted.dtype == torch.uint8
    w.check()
    w.add(65, as_float32=False, given_keys=False)
    w.check()
    w.add(1, as_float32=True, given_keys=False)
    w.check()


def _update_sq8(ix, rows, new_storage, keys, ids):
    """One `nlsh_csr_update_sq8` call on the arrays of `ix` (every old row kept) -> (sorted_out, gid_out, inv_out, src_out, uniq, offsets, bad, clamped)."""
    L, N, M, stride = _capi.lib(), int(ix.gid.shape[0]), int(rows.shape[0]), ix.row_stride
    n_out = N + M
    out = torch.empty((n_out, stride), dtype=torch.uint8, device="cuda")
    gid, src = torch.empty((n_out,), dtype=torch.int32, device="cuda"), torch.empty((n_out,), dtype=torch.int32, device="cuda")
    inv = torch.empty((n_out,), dtype=torch.float32, device="cuda")
    uniq, offs = torch.empty((n_out,), dtype=torch.int32, device="cuda"), torch.empty((n_out + 1,), dtype=torch.int32, device="cuda")
    nb, flags = torch.zeros((1,), dtype=torch.int32, device="cuda"), torch.zeros((2,), dtype=torch.int32, device="cuda")
    wb = L.nlsh_csr_update_workspace(N, ix.n_buckets, M)
    ws = torch.empty((wb,), dtype=torch.uint8, device="cuda")
    _capi.check(L.nlsh_csr_update_sq8(
        _capi.ptr(ix.corpus_sorted), _capi.ptr(ix._qlo), _capi.ptr(ix._qstep), stride, ix.dim, _capi.ptr(ix.gid), _capi.ptr(ix.inv_norm),
        _capi.ptr(ix.uniq_keys), _capi.ptr(ix.offsets), N, ix.n_buckets, None, N, _capi.ptr(rows), new_storage, rows.stride(0), _capi.ptr(keys),
        _capi.ptr(ids), M, _capi.ptr(out), stride, _capi.ptr(gid), _capi.ptr(inv), _capi.ptr(src), _capi.ptr(uniq), _capi.ptr(offs), _capi.ptr(nb),
        _capi.ptr(flags[0:1]), _capi.ptr(flags[1:2]), _capi.ptr(ws), wb, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    b = int(nb.item())
    return (out, gid, inv, src, uniq[:b], offs[:b + 1]) + tuple(flags.cpu().tolist())


@pytest.mark.parametrize("d", [7, 100])
def test_sq8_update_encodes_new_rows_of_every_storage(d):
    """`nlsh_csr_update_sq8` through the C ABI (the facade encodes float rows before the call, so it only reaches codes): float32 and
    float16 new rows, aligned and strided off by one element, give word for word the arrays of the call that is handed their codes."""
    from nlsh_amd.indexer import Indexer
    N, M = 900, 130
    rng = np.random.default_rng(d)
    X = real_rows(N, d, rng)
    keys_old = dev(rng.integers(-5, 6, size=N).astype(np.int32))
    keys_new = dev(rng.integers(-7, 8, size=M).astype(np.int32))
    ids_new = dev(np.arange(5000, 5000 + M, dtype=np.int32))
    ix = Indexer(_hasher(d), dev(X), _dist("cosine"), storage="sq8", corpus_keys=keys_old, compat=False)
    lo, step = (t.cpu() for t in ix.quantiser)
    Rn = real_rows(M, d, rng)
    Rn[3], Rn[50, d - 1] = Rn[3] * 100 + 50, np.float32(-6e4)                   # two rows that saturate (finite in float16 too)
    for dtype, code in ((torch.float32, _capi.STORE_F32), (torch.float16, _capi.STORE_F16)):
        src = torch.from_numpy(Rn).to(dtype)
        codes, clamped = rule_encode(src, lo, step)
        own = _update_sq8(ix, codes.cuda(), _capi.STORE_U8, keys_new, ids_new)
        assert own[6] == -1 and own[7] == 0
        new_at = own[3] < 0
        assert torch.equal(own[0][new_at][:, :d].cpu(), codes[(~own[3][new_at]).long().cpu()])
        wide = torch.zeros((M, d + 5), dtype=dtype, device="cuda")
        wide[:, 1:d + 1] = src.cuda()
        for rows in (src.cuda(), wide[:, 1:d + 1]):
            got = _update_sq8(ix, rows, code, keys_new, ids_new)
            assert got[6] == -1 and got[7] == int(clamped.sum()) >= 2
            for i, (a, b) in enumerate(zip(got[:6], own[:6])):
                _same(a, b, (dtype, i))
    bad = torch.from_numpy(Rn).clone()
    bad[99, 0], bad[77, d - 1] = float("nan"), float("inf")
    assert _update_sq8(ix, bad.cuda(), _capi.STORE_F32, keys_new, ids_new)[6] == 77


# ---------------------------------------------------------------------------------------------- refusals
def test_non_finite_rows_are_refused_by_name_and_change_nothing():
    from nlsh_amd.indexer import Indexer
    d, N = 20, 600
    rng = np.random.default_rng(9)
    X = real_rows(N, d, rng)
    hashing = _hasher(d)
    q = dev(real_rows(32, d, rng, special=False))
    keys = rng.integers(0, 20, size=N).astype(np.int32)
    good = Indexer(hashing, dev(X), _dist("l2"), storage="sq8", corpus_keys=dev(keys))
    before = good.query_tensors(q, k=5, hash_times=2, seed=1)
    arrays = {name: getattr(good, name).clone() for name in ("corpus_sorted", "gid", "perm", "uniq_keys", "offsets", "corpus_keys", "_qlo", "_qstep")}
    for i, v in enumerate([float("nan"), float("inf"), float("-inf")]):
        Y = X.copy()
        rows = sorted({(37 * i + 11) % N, N - 1 - i})
        for r in rows:
            Y[r, (3 * i) % d] = v
        for quantiser in (None, good.quantiser):                     # refused by the training pass, and by the encode under a given quantiser
            with pytest.raises(ValueError, match=rf"corpus row {rows[0]} holds a NaN or an infinity.*storage='sq8'"):
                Indexer(hashing, dev(Y), _dist("l2"), storage="sq8", corpus_keys=dev(keys), quantiser=quantiser)
        with pytest.raises(ValueError, match=rf"added row {rows[0]} holds"):
            good.add(dev(Y), keys=dev(keys))
        calls = repr(hashing._calls)
        with pytest.raises(ValueError, match=rf"added row {rows[0]} holds"):
            good.add(dev(Y))                                         # keys from the hash: refused BEFORE any encode
        assert repr(hashing._calls) == calls, "a refused add leaves the hasher's call counter alone"
        assert good.generation == 0
        for name, t in arrays.items():
            _same(getattr(good, name), t, name)
        assert_same_results(good.query_tensors(q, k=5, hash_times=2, seed=1), before, "after a refusal")
    with pytest.raises(ValueError, match=r"added rows must be float32 or uint8 \(codes\)"):
        good.add(dev(X).to(torch.float64), keys=dev(keys))
    with pytest.raises(NotImplementedError, match="storage='sq8'"):
        good.range_query(q, 1.0)
    with pytest.raises(NotImplementedError, match="storage='sq8'"):
        good.range_tensors(q, 1.0)


# ---------------------------------------------------------------------------------------------- the derived error bound
def test_distances_stay_within_half_a_step_of_the_original_rows():
    """The only test with a tolerance, and the tolerance is derived: ||x - deq(enc(x))||_2 <= 0.5 ||step||_2 for a row inside the trained
    range (each element is off by at most half its step), so by the triangle inequality an sq8 L2 distance differs from the float32
    distance to the ORIGINAL row by at most that -- plus the project's 2e-5 float32 tolerance on the distance itself.  |lo[j]| <= 16 *
    (hi[j] - lo[j]) keeps the float32 roundings inside the rule (relative 2^-24 of values below 17 ranges = 4335 steps: < 3e-4 of a step)
    under the 1.001.  Observed on the MI355X: the largest error 0.083 against a first term of 0.182, ratio 0.455 (printed below)."""
    from nlsh_amd.indexer import Indexer
    N, d, Q, k = 20000, 32, 256, 10
    rng = np.random.default_rng(77)
    scale = rng.uniform(0.05, 4.0, size=d)
    X = (rng.standard_normal((N, d)) * scale + rng.uniform(-2, 2, size=d) * scale).astype(np.float32)
    lo, step = sq8_train(X)
    assert (np.abs(lo) <= 16 * (step.astype(np.float64) * 255)).all()
    qv = (rng.standard_normal((Q, d)) * scale).astype(np.float32)
    hashing = _hasher(d, H=8)
    ix = Indexer(hashing, dev(X), _dist("l2"), storage="sq8", compat=False)
    dist, idx = ix.query_tensors(dev(qv), k=k, hash_times=8, seed=4)[:2]
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    found = idx >= 0
    assert found.sum() > Q * k // 2
    qi = np.nonzero(found)[0]
    exact = torch.nn.functional.pairwise_distance(torch.from_numpy(qv[qi]), torch.from_numpy(X[idx[found]])).numpy()      # float32, the metric's own form
    bound = 0.5 * np.linalg.norm(step.astype(np.float64)) * 1.001 + 2e-5 * np.maximum(1.0, exact)
    err = np.abs(dist[found].astype(np.float64) - exact)
    print(f"sq8 distance error: max {err.max():.5f}, bound's first term {0.5 * np.linalg.norm(step.astype(np.float64)):.5f}, "
          f"max ratio {(err / (0.5 * np.linalg.norm(step.astype(np.float64)))).max():.3f}")
    assert (err <= bound).all()
