"""Float16 / uint8 corpus storage against ITS DEFINITION: `Indexer(hashing, corpus, dist, storage=T)` is, word for word, the float32
index over the dequantised rows `S.float()` -- every index array, every distance bit, id, candidate count and result list.  The
reference is always the existing float32 path (`algo="tiled"` forced on the twin) on `S.float()` with the same `corpus_keys=`, never the
code under test, and every comparison is `torch.equal` on raw bits: no tolerance anywhere.  The conversion rule's reference is the numpy
restatement in tests/test_corpus_storage_cpu.py."""
import numpy as np
import pytest
import torch

from helpers import dev, make_hashing
from helpers import task_table as _task_table
from nlsh_amd import _capi, synth
from test_corpus_storage_cpu import convert, first_bad_row

pytestmark = pytest.mark.gpu

STORAGES = ("float16", "uint8")
NP = {"float16": np.float16, "uint8": np.uint8}
TORCH = {"float16": torch.float16, "uint8": torch.uint8}
PER16 = {"float16": 8, "uint8": 16}            # elements per 16 bytes: the pitch granularity
INDEX_ARRAYS = ("corpus_keys", "perm", "gid", "uniq_keys", "offsets", "inv_norm")


def _dist(metric):
    from nlsh_amd.data import Glove, SIFT
    return SIFT.distance if metric == "l2" else Glove.distance


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
        assert torch.equal(_bits(a), _bits(b)), what


CENTRE = {None: (0.0, 1.0), "float16": (0.0, 4.0), "uint8": (127.5, 74.0)}     # (mean, spread) of the values `stored` draws


def _hasher(d, H=16, compat=False, storage=None):
    """A seeded MLP hasher whose first layer standardises the storage's value range (uint8 rows are all-positive: without it every row
    and every query would land in one bucket)."""
    Ws, bs = synth.make_weights([d, 32, H], seed=d)
    mean, spread = CENTRE[storage]
    Ws[0] = (Ws[0] / spread).astype(np.float32)
    bs[0] = (bs[0] - Ws[0].sum(1) * mean).astype(np.float32)
    return make_hashing(d, (32,), H, Ws, bs, compat=compat)


def _raw(t):
    """A stored tensor by its bits."""
    return t.contiguous().view(torch.int16) if t.dtype == torch.float16 else t


def stored(storage, n, d, rng, special=True):
    """[n, d] values AS STORED (numpy, the storage's dtype).  The first rows are the edge values: uint8 -- all 0, all 255, alternating
    0 / 255; float16 -- subnormals, +-65504, -0.0, +-2^-24.  Finite data only."""
    if storage == "uint8":
        S = rng.integers(0, 256, size=(n, d)).astype(np.uint8)
        if special and n >= 4:
            S[0], S[1] = 0, 255
            S[2] = (np.arange(d) % 2) * 255
            S[3] = 255 - S[2]
    else:
        S = (rng.standard_normal((n, d)) * 4).astype(np.float16)
        if special and n >= 6:
            S[0] = (np.arange(d) % 1023 + 1).astype(np.uint16).view(np.float16)       # subnormals: bit patterns 1..1023
            S[1] = np.where(np.arange(d) % 2, -65504.0, 65504.0).astype(np.float16)
            S[2] = np.float16(-0.0)
            S[3] = np.where(np.arange(d) % 2, -(2.0 ** -24), 2.0 ** -24).astype(np.float16)
            S[4] = np.float16(65504.0)
    assert np.isfinite(S.astype(np.float32)).all()
    return S


def queries_for(storage, Q, d, rng):
    q = rng.integers(0, 256, size=(Q, d)).astype(np.float32) if storage == "uint8" else (rng.standard_normal((Q, d)) * 4).astype(np.float32)
    return q + rng.standard_normal((Q, d)).astype(np.float32) * 0.25            # queries stay float32: nothing rounds them


def build_pair(hashing, source, S, storage, metric="l2", row_align=4, keys=None, **kw):
    """(typed index built from `source`, its float32 twin built from `S.float()`), same keys, the twin on the tiled schedule with the
    typed pitch (a pitch never changes a result; with it the two sorted copies have one shape)."""
    from nlsh_amd.indexer import Indexer
    ck = None if keys is None else dev(np.asarray(keys, np.int32))
    typed = Indexer(hashing, source, _dist(metric), storage=storage, row_align=row_align, corpus_keys=ck, **kw)
    twin = Indexer(hashing, dev(S).float(), _dist(metric), algo="tiled", row_align=max(row_align, PER16[storage]), corpus_keys=ck, **kw)
    return typed, twin


def assert_is_the_twin(typed, twin, storage, cells=(64, 256)):
    """Every array the definition names."""
    d = typed.dim
    assert typed.storage == storage and typed.corpus_sorted.dtype == TORCH[storage] and twin.corpus_sorted.dtype == torch.float32
    assert typed.row_stride % PER16[storage] == 0 and typed.row_stride >= d
    assert typed.row_stride == twin.row_stride and typed.n_buckets == twin.n_buckets
    for name in INDEX_ARRAYS:
        _same(getattr(typed, name), getattr(twin, name), name)
    _same(typed.bucket_order[:typed.n_buckets], twin.bucket_order[:twin.n_buckets], "bucket_order")
    _same(typed.corpus_sorted.float(), twin.corpus_sorted, "corpus_sorted.float()")
    assert not bool((_raw(typed.corpus_sorted[:, d:]) != 0).any()), "padding columns are stored as zero (+0)"
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


def assert_same_results(ra, rb, what):
    for i, name in enumerate(("dist", "idx", "ncand")):
        _same(ra[i], rb[i], (what, name))


# ---------------------------------------------------------------------------------------------- index arrays
@pytest.mark.parametrize("d", [1, 3, 4, 7, 8, 15, 16, 17, 100, 128, 260, 1024])
def test_index_arrays_equal_the_float32_twins(d):
    """Both storages, the default pitch and row_align=32, sources of every dtype as contiguous, strided and misaligned views; keys from
    the hash of the dequantised rows (N > HASH_BATCH: the chunked encode) and given keys; one query batch through each pair."""
    from nlsh_amd.indexer import HASH_BATCH
    N, Q = 2000, 64
    for si, storage in enumerate(STORAGES):
        rng = np.random.default_rng(100 * d + si)
        hashing = _hasher(d, storage=storage)
        S = stored(storage, N, d, rng)
        q = dev(queries_for(storage, Q, d, rng))
        # given keys are drawn from the keys the queries hash to, so that the query batch below finds candidates
        pool = np.unique(np.r_[hashing.hash_device(q, n=1)[0].reshape(-1).cpu().numpy(), np.arange(100, 104)]).astype(np.int32)
        given = rng.choice(pool, size=N).astype(np.int32)
        wide = np.zeros((N, d + 3), NP[storage])
        wide[:, 1:d + 1] = S
        wide32 = np.zeros((N, d + 5), np.float32)
        wide32[:, 3:d + 3] = S.astype(np.float32)
        sources = {"contiguous": dev(S), "strided, off by one element": dev(wide)[:, 1:d + 1], "float32, strided": dev(wide32)[:, 3:d + 3]}
        if storage == "float16":                                                # uint8 -> float16 is exact as well
            S8 = stored("uint8", N, d, rng)
            sources["uint8 rows"] = dev(S8)
        else:                                                                   # ... and so is float16 -> uint8 on integers in [0, 255]
            sources["float16 rows"] = dev(S.astype(np.float16))
            sources["float16 rows, strided, off by one element"] = dev(wide.astype(np.float16))[:, 1:d + 1]
        for name, src in sources.items():
            for row_align in (4, 32):
                Sx = S8.astype(np.float16) if name == "uint8 rows" else S
                typed, twin = build_pair(hashing, src, Sx, storage, metric="cosine" if row_align == 32 else "l2", row_align=row_align, keys=given)
                assert_is_the_twin(typed, twin, storage)
                assert torch.equal(_raw(typed.corpus_sorted[:, :d].cpu()), _raw(torch.from_numpy(Sx)[typed.perm.long().cpu()])), (name, "stored bits")
                ra = typed.query_tensors(q, k=10, hash_times=4, seed=3)
                assert typed.last_query_path == "two_step" and typed.last_algo == _capi.SCAN_BUCKET_TILED
                assert int(ra[2].sum()) > 0
                assert_same_results(ra, twin.query_tensors(q, k=10, hash_times=4, seed=3), (storage, name, row_align))
    # keys from the hash: the chunked encode of the dequantised rows is the twin's one encode of S.float()
    n_big = HASH_BATCH + 904
    for si, storage in enumerate(STORAGES):
        rng = np.random.default_rng(7 * d + si)
        S = stored(storage, n_big, d, rng)
        typed, twin = build_pair(_hasher(d, storage=storage), dev(S), S, storage)
        assert_is_the_twin(typed, twin, storage, cells=(64,))


def test_keys_come_from_the_rounded_rows_not_from_the_callers_float32():
    """A float32 source that float16 rounds: the bucket keys are those of the ROUNDED rows (the twin hashes `S.float()`), and the
    stored bits are the CPU rule's (round to nearest even)."""
    d, N = 24, 5000
    rng = np.random.default_rng(5)
    X = (rng.standard_normal((N, d)) * 3).astype(np.float32)
    X[:8, :4] = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2049, 2051], np.float32)          # ties between float16 neighbours
    X[8, :4] = np.array([65519.996, -65519.996, 2.0 ** -25, 1.5 * 2.0 ** -24], np.float32)
    S = convert(X, "float16")
    hashing = _hasher(d, storage="float16")
    typed, twin = build_pair(hashing, dev(X), S, "float16")
    assert_is_the_twin(typed, twin, "float16", cells=(64,))
    assert torch.equal(_raw(typed.corpus_sorted[:, :d].cpu()), _raw(torch.from_numpy(S)[typed.perm.long().cpu()]))
    from nlsh_amd.indexer import Indexer
    unrounded = Indexer(hashing, dev(X), _dist("l2"), algo="tiled")
    assert not torch.equal(unrounded.corpus_keys, typed.corpus_keys)            # (the rounding really moves some keys: the test can tell)


@pytest.mark.parametrize("d", [1, 3, 7, 17, 100, 260, 1024])
def test_inv_norm_bits_do_not_depend_on_the_pitch(d):
    """The typed pitch is wider than the float32 default (8 / 16 / 32 elements against 4): the sum of squares only gains chunks of zeros,
    so `inv_norm` has the bits of the float32 index at ITS default pitch -- compared here, not argued."""
    from nlsh_amd.indexer import Indexer
    N, wider = 1500, False
    for si, storage in enumerate(STORAGES):
        rng = np.random.default_rng(31 * d + si)
        S = stored(storage, N, d, rng)
        keys = dev(rng.integers(-9, 9, size=N).astype(np.int32))
        hashing = _hasher(d, storage=storage)
        plain = Indexer(hashing, dev(S).float(), _dist("cosine"), algo="tiled", corpus_keys=keys)       # row_align 4: the float32 default
        assert plain.row_stride == (d + 3) // 4 * 4
        for row_align in (4, 32):
            typed = Indexer(hashing, dev(S), _dist("cosine"), storage=storage, corpus_keys=keys, row_align=row_align)
            assert typed.row_stride >= plain.row_stride
            wider = wider or typed.row_stride > plain.row_stride
            for name in ("inv_norm", "gid", "perm", "offsets"):
                _same(getattr(typed, name), getattr(plain, name), (storage, row_align, name))
    assert wider or d % 32 == 0, "the test compares pitches that differ"


# ---------------------------------------------------------------------------------------------- the C ABI between storages
CODE = {"float32": _capi.STORE_F32, "float16": _capi.STORE_F16, "uint8": _capi.STORE_U8}
ALL_TORCH = {"float32": torch.float32, **TORCH}
ALL_PER16 = {"float32": 4, **PER16}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gather_typed(src, src_storage, dst_storage, d, perm, stride, want_inv=True):
    n = perm.shape[0]
    out = torch.full((n, stride), 7, dtype=ALL_TORCH[dst_storage], device="cuda")
    inv = torch.empty((n,), dtype=torch.float32, device="cuda") if want_inv else None
    gid = torch.empty((n,), dtype=torch.int32, device="cuda")
    bad = torch.zeros((1,), dtype=torch.int32, device="cuda")
    _capi.check(_capi.lib().nlsh_gather_rows_typed(_capi.ptr(src), CODE[src_storage], src.stride(0), d, _capi.ptr(perm), n, _capi.ptr(out),
                                                   CODE[dst_storage], stride, _capi.ptr(inv), _capi.ptr(gid), 5, _capi.ptr(bad), _stream()))
    return out, inv, gid, int(bad.item())


@pytest.mark.parametrize("d", [3, 16, 100, 130])
def test_typed_gather_between_every_pair_of_storages(d):
    """`nlsh_gather_rows_typed` for all nine (source, destination) pairs on integers in [0, 255] (exact in every storage), aligned sources
    (one load per chunk) and strided, misaligned ones (element loads): the stored rows are the permuted values in the destination's
    type, zero padded; gid and the first-bad word are right; `inv_norm` has the bits of `nlsh_gather_rows` at the float32 default pitch."""
    n = 700
    rng = np.random.default_rng(d)
    V = rng.integers(0, 256, size=(n, d)).astype(np.float32)
    V[0], V[1] = 0, 255
    perm = dev(rng.permutation(n).astype(np.int32))
    s4 = (d + 3) // 4 * 4
    ref = torch.empty((n, s4), dtype=torch.float32, device="cuda")
    ref_inv = torch.empty((n,), dtype=torch.float32, device="cuda")
    _capi.check(_capi.lib().nlsh_gather_rows(_capi.ptr(dev(V)), d, d, _capi.ptr(perm), n, _capi.ptr(ref), s4, _capi.ptr(ref_inv), None, 0, _stream()))
    for src_storage in ALL_TORCH:
        wide = torch.zeros((n, d + 8 + 3), dtype=ALL_TORCH[src_storage], device="cuda")
        wide[:, 1:d + 1] = dev(V).to(ALL_TORCH[src_storage])
        aligned = torch.zeros((n, (d + 15) // 16 * 16), dtype=ALL_TORCH[src_storage], device="cuda")       # rows on 16-byte boundaries in every storage
        aligned[:, :d] = dev(V).to(ALL_TORCH[src_storage])
        for dst_storage in ALL_TORCH:
            stride = (d + ALL_PER16[dst_storage] - 1) // ALL_PER16[dst_storage] * ALL_PER16[dst_storage]
            for src in (aligned[:, :d], wide[:, 1:d + 1]):
                out, inv, gid, bad = _gather_typed(src, src_storage, dst_storage, d, perm, stride)
                what = (src_storage, dst_storage, src.data_ptr() % 16)
                assert bad == -1, what
                assert torch.equal(out[:, :d].float(), ref[:, :d]) and not bool((_raw(out[:, d:]) != 0).any()), what
                assert torch.equal(gid, perm + 5), what
                _same(inv, ref_inv, what)
    # a float16 source that uint8 cannot take: reported by its SOURCE row, whatever the permutation
    H = dev(V).half()
    H[123, d - 1] = 0.5
    H[400, 0] = 300.0
    for src in (H, H[:, :d]):
        assert _gather_typed(src, "float16", "uint8", d, perm, (d + 15) // 16 * 16)[3] == 123
    assert _gather_typed(H, "float16", "float32", d, perm, s4)[3] == -1          # float16 -> float32 takes everything


def _update_typed(ix, storage, rows, new_storage, keys, ids):
    """One `nlsh_csr_update_typed` call on the arrays of `ix` (every old row kept) -> (sorted_out, gid_out, inv_out, src_out, uniq, offsets, bad)."""
    L, N, M, stride = _capi.lib(), int(ix.gid.shape[0]), int(rows.shape[0]), ix.row_stride
    n_out = N + M
    out = torch.empty((n_out, stride), dtype=ALL_TORCH[storage], device="cuda")
    gid, src = torch.empty((n_out,), dtype=torch.int32, device="cuda"), torch.empty((n_out,), dtype=torch.int32, device="cuda")
    inv = torch.empty((n_out,), dtype=torch.float32, device="cuda")
    uniq, offs = torch.empty((n_out,), dtype=torch.int32, device="cuda"), torch.empty((n_out + 1,), dtype=torch.int32, device="cuda")
    nb, bad = torch.zeros((1,), dtype=torch.int32, device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
    wb = L.nlsh_csr_update_workspace(N, ix.n_buckets, M)
    ws = torch.empty((wb,), dtype=torch.uint8, device="cuda")
    _capi.check(L.nlsh_csr_update_typed(
        _capi.ptr(ix.corpus_sorted), CODE[storage], stride, ix.dim, _capi.ptr(ix.gid), _capi.ptr(ix.inv_norm), _capi.ptr(ix.uniq_keys),
        _capi.ptr(ix.offsets), N, ix.n_buckets, None, N, _capi.ptr(rows), CODE[new_storage], rows.stride(0), _capi.ptr(keys), _capi.ptr(ids), M,
        _capi.ptr(out), stride, _capi.ptr(gid), _capi.ptr(inv), _capi.ptr(src), _capi.ptr(uniq), _capi.ptr(offs), _capi.ptr(nb), _capi.ptr(bad),
        _capi.ptr(ws), wb, _stream()))
    torch.cuda.synchronize()
    b = int(nb.item())
    return out, gid, inv, src, uniq[:b], offs[:b + 1], int(bad.item())


@pytest.mark.parametrize("d", [7, 100])
def test_typed_update_converts_new_rows_of_every_storage(d):
    """`nlsh_csr_update_typed` through the C ABI with new rows of EVERY storage into an index of every storage (the facade converts float32
    rows before the call, so it only reaches new_storage == storage): all nine pairs give, word for word, the arrays of the call that is
    handed the rows in the index's own storage; for the float32 index that call is checked against `nlsh_csr_update` itself."""
    from nlsh_amd.indexer import Indexer
    N, M = 900, 130
    rng = np.random.default_rng(d)
    V = rng.integers(0, 256, size=(N, d)).astype(np.float32)
    R = rng.integers(0, 256, size=(M, d)).astype(np.float32)
    keys_old = dev(rng.integers(-5, 6, size=N).astype(np.int32))
    keys_new = dev(rng.integers(-7, 8, size=M).astype(np.int32))
    ids_new = dev(np.arange(5000, 5000 + M, dtype=np.int32))
    for storage in ALL_TORCH:
        ix = Indexer(_hasher(d), dev(V).to(ALL_TORCH[storage]), _dist("cosine"), storage=storage, corpus_keys=keys_old, compat=False)
        own = _update_typed(ix, storage, dev(R).to(ALL_TORCH[storage]), storage, keys_new, ids_new)
        assert own[6] == -1 and own[0].dtype == ALL_TORCH[storage]
        if storage == "float32":
            ix.update(add=dev(R), add_ids=ids_new, add_keys=keys_new)                   # `nlsh_csr_update`, the float32 kernel
            for got, want in zip(own[:3] + own[4:6], (ix.corpus_sorted, ix.gid, ix.inv_norm, ix.uniq_keys, ix.offsets)):
                _same(got, want, "float32 / float32 against nlsh_csr_update")
            ix = Indexer(_hasher(d), dev(V), _dist("cosine"), storage=storage, corpus_keys=keys_old, compat=False)
        for new_storage in ALL_TORCH:
            wide = torch.zeros((M, d + 5), dtype=ALL_TORCH[new_storage], device="cuda")
            wide[:, 1:d + 1] = dev(R).to(ALL_TORCH[new_storage])
            for rows in (dev(R).to(ALL_TORCH[new_storage]), wide[:, 1:d + 1]):                 # aligned, and strided off by one element
                got = _update_typed(ix, storage, rows, new_storage, keys_new, ids_new)
                assert got[6] == -1
                for i, (a, b) in enumerate(zip(got[:6], own[:6])):
                    _same(_raw(a), _raw(b), (storage, new_storage, i))
    # a float16 row that uint8 cannot take is reported by its index among the new rows
    ix = Indexer(_hasher(d), dev(V).to(torch.uint8), _dist("cosine"), storage="uint8", corpus_keys=keys_old, compat=False)
    H = dev(R).half()
    H[77, 0], H[99, d - 1] = 0.25, -1.0
    assert _update_typed(ix, "uint8", H, "float16", keys_new, ids_new)[6] == 77


# ---------------------------------------------------------------------------------------------- scan across task shapes
SIZES = (1, 2, 40, 41, 63, 64, 65, 255, 256, 257, 700)   # rows per bucket: single-stage tasks either side of rows * d4 <= 1024 (d = 100), 1..4 tiles, 2 and 3 segments
GROUPS = (1, 5, 11, 16, 17)                               # queries per bucket: a wave holds 1,0 / 2,1 / 3,2 / 4 of them; 17 = two groups
TINY = 48                                                 # a run of buckets of 1..6 rows: shared windows
SD, SQ = 100, 64


def _shape_world(storage, seed):
    rng = np.random.default_rng(seed)
    buckets = [(s, m) for s in SIZES for m in GROUPS] + [(1 + i % 6, 1 + i % 3) for i in range(TINY)]
    N = sum(s for s, _ in buckets)
    S = stored(storage, N, SD, rng)
    keys = np.repeat(np.arange(len(buckets), dtype=np.int32) * 3 - 200, [s for s, _ in buckets])
    order = rng.permutation(N)
    corpus_keys = np.empty(N, np.int32)
    corpus_keys[order] = keys
    first = {b: np.flatnonzero(corpus_keys == b * 3 - 200) for b in range(len(buckets))}
    ties = next(b for b, (s, m) in enumerate(buckets) if s == 256 and m == 17)
    S[first[ties]] = S[first[ties][0]]                              # a bucket of identical rows: the (distance, id) order decides
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
    return S, corpus_keys, buckets, dev(tab), dev(cnt), dev(queries_for(storage, SQ, SD, rng))


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("form", ["l2", "folded", "cosine"])
def test_scan_equals_the_twin_on_every_task_shape(form, storage):
    metric = "cosine" if form == "cosine" else "l2"
    S, corpus_keys, buckets, keys, nkeys, q = _shape_world(storage, seed=11 + len(form))
    kw = {"l2_form": "folded"} if form == "folded" else {}
    typed, twin = build_pair(_hasher(SD, storage=storage), dev(S), S, storage, metric=metric, keys=corpus_keys, compat=False, **kw)
    assert_is_the_twin(typed, twin, storage)
    P = keys.shape[1]
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
    assert_same_results(ra, rb, (form, storage, "window 0"))
    _same(ra[3], rb[3], "keys64")
    for k in (1, 64, 65, 100, 256):
        assert_same_results(typed.scan_tensors(q, keys, nkeys, k=k), twin.scan_tensors(q, keys, nkeys, k=k), (form, storage, "window 0", k))
    # ---- shared windows: the run of tiny buckets (and every other bucket of <= window rows) is packed
    for window, ks in ((64, (1, 10, 64, 65, 256)), (128, (10, 100)), (256, (10, 100))):
        typed.window_rows = twin.window_rows = window
        for k in ks:
            ra, rb = typed.scan_tensors(q, keys, nkeys, k=k), twin.scan_tensors(q, keys, nkeys, k=k)
            assert typed.last_window == window and twin.last_window == window
            assert_same_results(ra, rb, (form, storage, window, k))
        assert int(typed.last_status.cpu()[0]) < len(nq)                        # fewer tasks than buckets: windows were shared
    # the ties bucket: its ids come out ascending within one distance
    dist, idx = ra[0].cpu().numpy(), ra[1].cpu().numpy()
    for row_d, row_i in zip(dist, idx):
        same = (row_d[1:] == row_d[:-1]) & (row_i[1:] >= 0)
        assert np.all(row_i[1:][same] > row_i[:-1][same])


def test_the_typed_call_with_float32_storage_is_the_untyped_call():
    from nlsh_amd.indexer import Indexer, _SCAN_ARGS_AFTER_QUERIES, _SCAN_ARGS_BEFORE_QUERIES
    S, corpus_keys, _, keys, nkeys, q = _shape_world("float16", seed=3)
    L, k, P = _capi.lib(), 10, keys.shape[1]
    for algo, code in (("query", _capi.SCAN_QUERY_MAJOR), ("bucket", _capi.SCAN_BUCKET_MAJOR), ("tiled", _capi.SCAN_BUCKET_TILED)):
        ix = Indexer(_hasher(SD), dev(S).float(), _dist("l2"), algo=algo, corpus_keys=dev(corpus_keys), compat=False)
        want = ix.scan_tensors(q, keys, nkeys, k=k)
        max_tasks, window = ix._last_max_tasks, ix.last_window
        out_dist, pack, out_idx, ncand, status, _ = ix._outputs(SQ, k, q.device)
        ws = torch.zeros((L.nlsh_scan_workspace(SQ, P, k, max_tasks, ix.n_buckets, SD),), dtype=torch.uint8, device=q.device)
        f = ix._scan_fields(SQ, SD, keys, nkeys, k, code, max_tasks, out_dist, out_idx, None, ncand, status, ws, window)
        before = _SCAN_ARGS_BEFORE_QUERIES(f)
        _capi.check(L.nlsh_scan_topk_cells_phase_typed(before[0], _capi.STORE_F32, *before[1:], q.data_ptr(), q.stride(0), *_SCAN_ARGS_AFTER_QUERIES(f),
                                                       None, None, torch.cuda.current_stream().cuda_stream, _capi.PHASE_ALL))
        assert_same_results((out_dist, out_idx, ncand), want, algo)
        assert status.cpu().tolist()[1] == 0


# ---------------------------------------------------------------------------------------------- conversion and refusals
@pytest.mark.parametrize("storage", STORAGES)
def test_a_source_that_does_not_survive_is_refused_and_names_its_first_row(storage):
    from nlsh_amd.indexer import Indexer
    d, N = 20, 600
    rng = np.random.default_rng(9)
    S = stored(storage, N, d, rng)
    hashing = _hasher(d, storage=storage)
    q = dev(queries_for(storage, 32, d, rng))
    keys = rng.integers(0, 20, size=N).astype(np.int32)
    good = Indexer(hashing, dev(S), _dist("l2"), storage=storage, corpus_keys=dev(keys))
    before = good.query_tensors(q, k=5, hash_times=2, seed=1)
    arrays = {name: getattr(good, name).clone() for name in ("corpus_sorted", "gid", "perm", "uniq_keys", "offsets", "corpus_keys")}
    bad_values = ([65520.0, -1e30, 70000.0] if storage == "float16" else [0.5, -1.0, 256.0, float("nan"), float("inf"), 1e9])
    for i, v in enumerate(bad_values):
        X = S.astype(np.float32)
        rows = sorted({(37 * i + 11) % N, N - 1 - i})
        for r in rows:
            X[r, (3 * i) % d] = v
        assert first_bad_row(X, storage) == rows[0]
        with pytest.raises(ValueError, match=rf"corpus row {rows[0]} holds .*storage='{storage}'"):
            Indexer(hashing, dev(X), _dist("l2"), storage=storage, corpus_keys=dev(keys))
        with pytest.raises(ValueError, match=rf"added row {rows[0]} holds"):
            good.add(dev(X), keys=dev(keys))
        calls = repr(hashing._calls)
        with pytest.raises(ValueError, match=rf"added row {rows[0]} holds"):
            good.add(dev(X))                                        # keys from the hash: refused BEFORE any encode
        assert repr(hashing._calls) == calls, "a refused add leaves the hasher's call counter alone"
        # the refused update touched nothing: same arrays, same generation, same answers
        assert good.generation == 0
        for name, t in arrays.items():
            _same(getattr(good, name), t, name)
        assert_same_results(good.query_tensors(q, k=5, hash_times=2, seed=1), before, "after a refusal")
    # values that look dangerous and are fine: float16 takes infinities-free extremes, uint8 takes -0.0
    ok = S.astype(np.float32)
    ok[0, 0] = 65519.996 if storage == "float16" else -0.0
    fine = Indexer(hashing, dev(ok), _dist("l2"), storage=storage, corpus_keys=dev(keys))
    assert torch.equal(_raw(fine.corpus_sorted[:, :d].cpu()), _raw(torch.from_numpy(convert(ok, storage))[fine.perm.long().cpu()]))
    with pytest.raises(ValueError, match="added rows must be float32 or " + storage):
        good.add(dev(S).to(torch.float64), keys=dev(keys))


# ---------------------------------------------------------------------------------------------- facade
@pytest.mark.parametrize("storage", STORAGES)
def test_facade_results_equal_the_twins(storage):
    """`query()` lists and counts with the F7 short-list fallback (compat on and off), ranked probes, the candidate budget, hash_times > 64
    (the sliced scan) and `query_with_keys`; the typed index always takes the two-step route."""
    from nlsh_amd.indexer import Indexer
    d, N, Q, k = 32, 6000, 512, 10
    rng = np.random.default_rng(21)
    S = stored(storage, N, d, rng)
    S[N // 2:] = S[:N - N // 2]                                    # every row twice: distance ties across the corpus
    q = dev(queries_for(storage, Q, d, rng))
    for compat in (True, False):
        hashing = _hasher(d, H=10, compat=compat, storage=storage)
        typed = Indexer(hashing, dev(S), _dist("l2"), storage=storage, compat=compat)
        twin = Indexer(hashing, dev(S).float(), _dist("l2"), algo="tiled", compat=compat, row_align=PER16[storage])
        assert_is_the_twin(typed, twin, storage, cells=(64,))
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
        key_lists = [[int(v) for v in typed._uniq_host[(7 * i) % typed.n_buckets:][:1 + i % 5]] + ([123456] if i % 9 == 0 else []) for i in range(Q)]
        got, want = typed.query_with_keys(q, key_lists, k=k), twin.query_with_keys(q, key_lists, k=k)
        assert got[0] == want[0] and got[1] == want[1]
        _same(got[2], want[2], "query_with_keys dist")
        _same(got[3], want[3], "query_with_keys idx")


def test_generic_metric_reads_the_rows_as_the_index_holds_them():
    from nlsh_amd.indexer import Indexer
    d, N = 16, 800
    rng = np.random.default_rng(2)
    X = (rng.standard_normal((N, d)) * 3).astype(np.float32)
    S = convert(X, "float16")
    hashing = _hasher(d, H=6, compat=False, storage="float16")
    fn = lambda a, b: (a - b).abs().sum(-1)   # noqa: E731  (an unknown callable: the generic path)
    q = dev(queries_for("float16", 16, d, rng))
    typed = Indexer(hashing, dev(X), fn, storage="float16", metric="custom", compat=False)
    twin = Indexer(hashing, dev(S).float(), fn, metric="custom", compat=False)
    got, want = typed.query(q, k=5, hash_times=1), twin.query(q, k=5, hash_times=1)      # (one probe: the hard key, no draw)
    assert got == want and max(want[1]) >= 5


# ---------------------------------------------------------------------------------------------- mutation
class World:
    """A typed index, its float32 twin and the model of the rows they should hold (local order), mutated side by side: the typed index
    gets float32 or typed rows, the twin the dequantised rows."""

    def __init__(self, storage, metric, d, n, seed):
        from nlsh_amd.indexer import Indexer
        self.storage, self.metric, self.d = storage, metric, d
        self.rng = np.random.default_rng(seed)
        self.hashing = _hasher(d, H=8, storage=storage)
        self.S = self.values(n)
        self.ids = np.arange(n, dtype=np.int32)
        self.typed = Indexer(self.hashing, dev(self.S), _dist(metric), storage=storage, compat=False)
        self.twin = Indexer(self.hashing, dev(self.S).float(), _dist(metric), algo="tiled", compat=False, row_align=PER16[storage])
        self.keys = self.typed.corpus_keys.cpu().numpy()
        self.q = dev(queries_for(storage, 64, d, self.rng))

    def values(self, n):
        """Representable in the storage AND exact in float32 arithmetic of the hasher's input: small integers (uint8), quarters (float16)."""
        if self.storage == "uint8":
            return self.rng.integers(0, 256, size=(n, self.d)).astype(np.uint8)
        return (self.rng.integers(-64, 65, size=(n, self.d)) / 4).astype(np.float16)

    def add(self, n, as_float32, given_keys):
        rows = self.values(n)
        src = dev(rows.astype(np.float32)) if as_float32 else dev(rows)
        keys = dev(self.rng.choice(self.keys, size=n).astype(np.int32)) if given_keys and len(self.keys) else None
        ids = self.typed.add(src, keys=keys)
        ids2 = self.twin.add(dev(rows).float(), keys=keys)
        assert torch.equal(ids, ids2)
        self.S = np.concatenate([self.S, rows])
        self.ids = np.r_[self.ids, ids.cpu().numpy()].astype(np.int32)
        self.keys = self.typed.corpus_keys.cpu().numpy()

    def remove(self, ids):
        ids = np.asarray(ids, np.int64)
        n = self.typed.remove(ids.tolist())
        assert n == self.twin.remove(ids.tolist()) == int(np.isin(self.ids, ids).sum())
        stay = ~np.isin(self.ids, ids)
        self.S, self.ids = self.S[stay], self.ids[stay]
        self.keys = self.typed.corpus_keys.cpu().numpy()

    def update(self, n_add, ids_remove):
        rows = self.values(n_add)
        ids_remove = np.asarray(ids_remove, np.int64)
        a = self.typed.update(add=dev(rows), remove=ids_remove.tolist())
        b = self.twin.update(add=dev(rows).float(), remove=ids_remove.tolist())
        assert torch.equal(a[0], b[0]) and a[1] == b[1]
        stay = ~np.isin(self.ids, ids_remove)
        self.S, self.ids = np.concatenate([self.S[stay], rows]), np.r_[self.ids[stay], a[0].cpu().numpy()].astype(np.int32)
        self.keys = self.typed.corpus_keys.cpu().numpy()

    def check(self):
        from nlsh_amd.indexer import Indexer
        assert len(self.keys) == len(self.ids) == len(self.S)
        rebuilt = Indexer(self.hashing, dev(self.S), _dist(self.metric), storage=self.storage, compat=False, corpus_keys=dev(self.keys),
                          row_ids=dev(self.ids))
        for name in INDEX_ARRAYS + ("corpus_sorted",):
            _same(getattr(self.typed, name), getattr(rebuilt, name), ("rebuild", name))
        _same(self.typed.bucket_order[:self.typed.n_buckets], rebuilt.bucket_order[:rebuilt.n_buckets], "bucket_order")
        assert_is_the_twin(self.typed, self.twin, self.storage, cells=(64,))
        if len(self.ids):
            assert_same_results(self.typed.query_tensors(self.q, k=5, hash_times=4, seed=5), self.twin.query_tensors(self.q, k=5, hash_times=4, seed=5),
                                "after mutation")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_mutations_equal_the_typed_rebuild_and_the_mutated_twin(metric, storage):
    w = World(storage, metric, d=100, n=20000, seed=len(metric) + len(storage))
    w.add(300, as_float32=True, given_keys=False)
    w.check()
    w.remove(w.rng.choice(w.ids, size=500, replace=False))
    w.check()
    w.update(257, w.rng.choice(w.ids, size=100, replace=False))
    w.check()
    for step in range(10):
        kind = step % 3
        if kind == 0:
            w.add(int(w.rng.integers(1, 400)), as_float32=bool(step % 2), given_keys=bool(step % 4 == 0))
        elif kind == 1:
            w.remove(np.r_[w.rng.choice(w.ids, size=int(w.rng.integers(1, 300)), replace=False), [10 ** 8]])
        else:
            w.update(int(w.rng.integers(1, 200)), w.rng.choice(w.ids, size=int(w.rng.integers(1, 200)), replace=False))
    w.check()
    assert w.typed.generation == 13


@pytest.mark.parametrize("storage", STORAGES)
def test_an_emptied_index_is_refilled(storage):
    w = World(storage, "cosine", d=7, n=300, seed=4)
    w.remove(w.ids.copy())
    assert w.typed.n_buckets == 0 and w.typed.corpus_sorted.shape == (0, w.typed.row_stride) and w.typed.corpus_sorted.dtype == TORCH[storage]
    w.check()
    w.add(65, as_float32=False, given_keys=False)
    w.check()
    w.add(1, as_float32=True, given_keys=False)
    w.check()


# ---------------------------------------------------------------------------------------------- peak memory of the build
@pytest.mark.parametrize("storage", STORAGES)
def test_the_build_makes_no_float32_copy_of_the_corpus(storage):
    """Peak extra memory of the constructor: the sorted typed copy, the int32 arrays of the build (keys, perm, ids, the CSR arrays and
    the radix sort's scratch: bounded by 64 bytes per row, the float32 build has them too) and a few HASH_BATCH-row chunks.  A float32
    copy of these rows (N * d * 4 bytes) would more than double it."""
    from nlsh_amd.indexer import HASH_BATCH, Indexer
    N, d = 200_000, 128
    rng = np.random.default_rng(1)
    src = dev(stored(storage, N, d, rng, special=False))
    hashing = _hasher(d, storage=storage)
    Indexer(hashing, src[:HASH_BATCH + 1], _dist("l2"), storage=storage)          # (packed weights and the library's first-use allocations)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ix = Indexer(hashing, src, _dist("l2"), storage=storage)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    sorted_bytes = N * ix.row_stride * src.element_size()
    assert ix.corpus_sorted.numel() * ix.corpus_sorted.element_size() == sorted_bytes
    bound = sorted_bytes + 64 * N + 4 * HASH_BATCH * d * 4 + (8 << 20)
    print(f"storage={storage}: peak extra {peak / 2 ** 20:.1f} MiB, sorted copy {sorted_bytes / 2 ** 20:.1f} MiB, bound {bound / 2 ** 20:.1f} MiB, "
          f"a float32 copy {N * d * 4 / 2 ** 20:.1f} MiB")
    assert bound < sorted_bytes + N * d * 4, "the bound can tell a float32 copy"
    assert sorted_bytes <= peak <= bound
