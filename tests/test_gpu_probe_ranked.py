"""Likelihood-ranked multi-probe keys on the GPU: `nlsh_probe_ranked` on injected pre-activations, through the hasher
(`probes="ranked"`) and through the `Indexer`, each bitwise against the Python reference of tests/ranked_ref.py (no tolerance anywhere:
keys, counts and the fp32 costs are pinned bit for bit)."""
import numpy as np
import pytest
import torch

import ranked_ref as rr
from helpers import dev, make_hashing

pytestmark = pytest.mark.gpu

P_ALL = (1, 2, 7, 8, 64, 65, 128)      # 65 crosses one frontier entry per lane, 128 fills the frontier


def probe(z, codes, H, P, key_mode, n_multi_rows=None, want_cost=True):
    """One `nlsh_probe_ranked` call on device tensors -> (keys, nkeys, cost bits) as numpy arrays."""
    from nlsh_amd import _capi
    n = z.shape[0]
    keys = torch.full((n, P), -7, dtype=torch.int32, device=z.device)
    nkeys = torch.full((n,), -7, dtype=torch.int32, device=z.device)
    cost = torch.full((n, P), -7.0, dtype=torch.float32, device=z.device) if want_cost else None
    _capi.check(_capi.lib().nlsh_probe_ranked(_capi.ptr(z), z.stride(0), _capi.ptr(codes), n, H, key_mode, P,
                                              n if n_multi_rows is None else n_multi_rows, _capi.ptr(keys), _capi.ptr(nkeys),
                                              _capi.ptr(cost), torch.cuda.current_stream(z.device).cuda_stream))
    torch.cuda.synchronize()
    return keys.cpu().numpy(), nkeys.cpu().numpy(), None if cost is None else cost.cpu().numpy().view(np.uint32)


def assert_table(got, want, what):
    for name, g, w in zip(("keys", "nkeys", "cost"), got, want):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())


def rows_for_two_workgroups():
    from nlsh_amd import _capi
    return 2 * _capi.PROBE_RANKED_ROWS_PER_WORKGROUP + 1


# ---------------------------------------------------------------------------- the kernel on injected z
@pytest.mark.parametrize("key_mode", [rr.KEY_REF_INT16, rr.KEY_FULL])
@pytest.mark.parametrize("H", [1, 2, 3, 5, 8, 16, 17, 31, 32])
def test_random_rows_match_the_reference(H, key_mode):
    n = rows_for_two_workgroups()
    z = rr.random_rows(n, H, seed=H)
    codes = np.random.default_rng(1000 + H).integers(0, 1 << H, size=n, dtype=np.uint64).astype(np.uint32)   # any code, not only z's own
    zd, cd = dev(z), dev(codes.view(np.int32))
    for P in P_ALL:
        assert_table(probe(zd, cd, H, P, key_mode), rr.table(z, codes, H, P, key_mode), (H, P, key_mode))


@pytest.mark.parametrize("kind", ["ties", "absorbing"])
@pytest.mark.parametrize("H", [5, 17, 32])
def test_mass_ties_match_the_reference(kind, H):
    n = rows_for_two_workgroups()
    z = (rr.tie_rows if kind == "ties" else rr.absorbing_rows)(n, H, seed=7 * H)
    codes = rr.hard_codes(z, H)
    zd, cd = dev(z), dev(codes.view(np.int32))
    for P in (7, 65, 128):
        want = rr.table(z, codes, H, P, rr.KEY_FULL)
        assert_table(probe(zd, cd, H, P, rr.KEY_FULL), want, (kind, H, P))
        assert any(len(set(row[:c].tolist())) < c for row, c in zip(want[2], want[1])) or P <= 7      # the rows do tie


def test_all_zero_rows_enumerate_the_masks_in_order():
    H, P, n = 9, 128, 5
    z = np.zeros((n, H), dtype=np.float32)
    z[1::2] = -0.0
    codes = np.arange(n, dtype=np.uint32) * 37 % (1 << H)
    keys, nkeys, cost = probe(dev(z), dev(codes.view(np.int32)), H, P, rr.KEY_FULL)
    flips = np.array([int(format(m, "09b")[::-1], 2) for m in range(P)], dtype=np.uint32)       # sorted position i = bit index i = code bit H-1-i
    assert np.array_equal(keys.view(np.uint32), codes[:, None] ^ flips[None, :])
    assert np.array_equal(nkeys, np.full(n, P)) and not cost.any()


@pytest.mark.parametrize("H", [1, 2, 3])
def test_a_small_hash_is_exhausted(H):
    n, P = rows_for_two_workgroups(), 16
    z = rr.random_rows(n, H, seed=40 + H)
    codes = rr.hard_codes(z, H)
    for key_mode in (rr.KEY_REF_INT16, rr.KEY_FULL):
        keys, nkeys, cost = probe(dev(z), dev(codes.view(np.int32)), H, P, key_mode)
        assert np.array_equal(nkeys, np.full(n, 1 << H))
        for r in range(n):
            assert sorted(keys[r, :1 << H].tolist()) == list(range(1 << H)) and keys[r, 0] == codes[r]
        assert np.array_equal(cost[:, 1 << H:], np.full((n, P - (1 << H)), rr.INF_BITS)) and not keys[:, 1 << H:].any()
        assert_table((keys, nkeys, cost), rr.table(z, codes, H, P, key_mode), (H, key_mode))


def test_colliding_int16_keys_are_dropped_in_first_occurrence_order():
    H, n = 20, rows_for_two_workgroups()
    z = rr.random_rows(n, H, seed=5)
    z[0, :] = 5.0
    z[0, :4] = [0.1, -0.2, 0.3, -0.4]         # the cheapest flips sit in code bits 19..16, which a 16-bit key does not see
    z[1, 4:] *= 50.0                          # likewise on a random row
    codes = rr.hard_codes(z, H)
    zd, cd = dev(z), dev(codes.view(np.int32))
    for P in (16, 65, 128):
        want = rr.table(z, codes, H, P, rr.KEY_REF_INT16)
        assert want[1][0] < P and want[1][1] < P and want[1].min() >= 1
        assert_table(probe(zd, cd, H, P, rr.KEY_REF_INT16), want, P)
    assert rr.table(z[:1], codes[:1], H, 16, rr.KEY_REF_INT16)[1].tolist() == [1]       # sixteen subsets of four invisible bits: one key


def test_rows_past_n_multi_rows_hold_the_hard_key_alone():
    H, P, n = 12, 10, 13
    z = rr.random_rows(n, H, seed=9)
    codes = rr.hard_codes(z, H)
    for n_multi in (0, 6, n):
        got = probe(dev(z), dev(codes.view(np.int32)), H, P, rr.KEY_FULL, n_multi_rows=n_multi)
        assert_table(got, rr.table(z, codes, H, P, rr.KEY_FULL, n_multi_rows=n_multi), n_multi)
        assert np.array_equal(got[1], np.where(np.arange(n) < n_multi, P, 1))
        assert np.array_equal(got[0][n_multi:, 0], codes[n_multi:].view(np.int32)) and not got[0][n_multi:, 1:].any()


def test_rows_are_independent_of_their_batch_and_of_the_stride():
    H, P, n = 17, 65, 23
    wide = np.full((n, 40), np.nan, dtype=np.float32)         # the columns past H are never read
    wide[:, :H] = rr.absorbing_rows(n, H, seed=11)
    wide[::3, :H] = rr.random_rows(len(wide[::3]), H, seed=12)
    codes = rr.hard_codes(wide[:, :H], H)
    wd, cd = dev(wide), dev(codes.view(np.int32))
    view = wd[:, :H]
    assert view.stride(0) == 40
    whole = probe(view, cd, H, P, rr.KEY_FULL)
    assert_table(whole, rr.table(wide[:, :H], codes, H, P, rr.KEY_FULL), "strided")
    assert_table(probe(view.contiguous(), cd, H, P, rr.KEY_FULL), whole, "contiguous copy")
    for a, b in ((0, 1), (3, 10), (9, 23)):
        assert_table(probe(view[a:b], cd[a:b], H, P, rr.KEY_FULL), tuple(t[a:b] for t in whole), (a, b))
    keys, nkeys, _ = probe(view, cd, H, P, rr.KEY_FULL, want_cost=False)      # cost_out is optional
    assert np.array_equal(keys, whole[0]) and np.array_equal(nkeys, whole[1])


# ---------------------------------------------------------------------------- through the hasher
def _hasher(dims, compat, tanh=False, seed=3):
    from nlsh_amd import synth
    Ws, bs = synth.make_weights(dims, seed=seed, gain=3.0)
    return make_hashing(dims[0], dims[1:-1], dims[-1], Ws, bs, tanh=tanh, compat=compat)


@pytest.fixture(scope="module", params=[(16, 32, 12), (8, 640, 12)], ids=["lds", "streamed"])
def hasher_case(request):
    """(hasher, x, z, code) of one encoder: the pre-activations and hard codes are `forward_device`'s own, so no expf enters."""
    dims = list(request.param)
    h = _hasher(dims, compat=False)
    assert h.streamed() == (dims[1] > 632)
    x = dev(np.random.default_rng(21).standard_normal((150, dims[0])).astype(np.float32))
    z, _, code = h.forward_device(x)
    torch.cuda.synchronize()
    return h, x, z.cpu().numpy(), code.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("P", [1, 10, 128])
def test_ranked_hashing_equals_the_reference_on_the_encoders_own_z(hasher_case, P):
    from nlsh_amd import _capi
    h, x, z, code = hasher_case
    H = z.shape[1]
    keys, nkeys = h.hash_device(x, n=P, probes="ranked")
    want = rr.table(z, code, H, P, _capi.KEY_FULL)
    assert np.array_equal(keys.cpu().numpy(), want[0]) and np.array_equal(nkeys.cpu().numpy(), want[1])
    assert np.array_equal(nkeys.cpu().numpy(), np.full(len(z), P))                   # full-width keys, 2^H >= P: P distinct buckets
    # slot 0 is the sampled mode's slot 0; the seed does not enter; the sampled mode is what it was
    skeys, snkeys = h.hash_device(x, n=P, seed=5, probes="sampled")
    assert torch.equal(skeys[:, 0], keys[:, 0])
    calls = repr(h._calls)
    k2, n2 = h.hash_device(x, n=P, seed=99, row0=1234, probes="ranked")
    assert torch.equal(k2, keys) and torch.equal(n2, nkeys)
    k2, n2 = h.hash_device(x, n=P, probes="ranked")
    assert torch.equal(k2, keys) and torch.equal(n2, nkeys) and repr(h._calls) == calls      # no seed is drawn from the call counter
    dkeys, dnkeys = h.hash_device(x, n=P, seed=5)
    assert torch.equal(dkeys, skeys) and torch.equal(dnkeys, snkeys)
    assert h.probes == "sampled"
    # the host form, the attribute, `out=` and the trailing-batch rule
    sets = h.hash(x[:20], n=P, probes="ranked")
    assert sets == [set((want[0][r, :P].astype(np.int64) & 0xFFFFFFFF).tolist()) for r in range(20)]
    out = (torch.zeros((len(z), P), dtype=torch.int32, device=x.device), torch.zeros((len(z),), dtype=torch.int32, device=x.device))
    h.probes = "ranked"
    try:
        k3, n3 = h.hash_device(x, n=P, n_multi_rows=100, out=out)
    finally:
        h.probes = "sampled"
    assert k3 is out[0] and n3 is out[1]
    want_multi = rr.table(z, code, H, P, _capi.KEY_FULL, n_multi_rows=100)
    assert np.array_equal(k3.cpu().numpy(), want_multi[0]) and np.array_equal(n3.cpu().numpy(), want_multi[1])


def test_ranked_hashing_with_the_tanh_head_and_int16_keys():
    """tanh: p = sigmoid(2z), the same order; compat keys of a 20-bit code collide and are de-duplicated like the reference's."""
    from nlsh_amd import _capi
    h = _hasher([16, 32, 20], compat=True, tanh=True)
    x = dev(np.random.default_rng(22).standard_normal((60, 16)).astype(np.float32))
    z, _, code = h.forward_device(x)
    keys, nkeys = h.hash_device(x, n=32, probes="ranked")
    want = rr.table(z.cpu().numpy(), code.cpu().numpy().view(np.uint32), 20, 32, _capi.KEY_REF_INT16)
    assert np.array_equal(keys.cpu().numpy(), want[0]) and np.array_equal(nkeys.cpu().numpy(), want[1])


def test_ranked_hashing_needs_eval_mode_for_batchnorm_encoders():
    from nlsh_amd import _capi
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.hashings import MultivariateBernoulli
    h = MultivariateBernoulli(MultiLayerRelu(8, [16], with_batchnorm=True), 6, None, compat=False)
    h.train_mode(True)
    x = dev(np.random.default_rng(2).standard_normal((32, 8)).astype(np.float32))
    with pytest.raises(_capi.NlshHipError) as e:
        h.hash_device(x, n=4, probes="ranked")
    assert e.value.code == _capi.E_UNSUPPORTED and "eval mode" in str(e.value)
    assert h.hash_device(x, n=4)[0].shape == (32, 4)           # the sampled mode still hashes in train mode


# ---------------------------------------------------------------------------- through the Indexer
@pytest.fixture(scope="module")
def index_case():
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    rng = np.random.default_rng(31)
    corpus = rng.standard_normal((4096, 16)).astype(np.float32)
    queries = dev(rng.standard_normal((200, 16)).astype(np.float32))
    h = _hasher([16, 32, 8], compat=False)
    ix = Indexer(h, dev(corpus), SIFT.distance, compat=False)
    z, _, code = h.forward_device(queries)
    torch.cuda.synchronize()
    return ix, h, queries, z.cpu().numpy(), code.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("P", [10, 100])
def test_indexer_queries_probe_the_reference_keys(index_case, P):
    from nlsh_amd import _capi
    ix, h, q, z, code = index_case
    keys, nkeys, _ = rr.table(z, code, 8, P, _capi.KEY_FULL)
    dist, idx, ncand, _ = ix.query_tensors(q, k=10, hash_times=P, probes="ranked")
    wdist, widx, wncand, _ = ix.scan_tensors(q, dev(keys), dev(nkeys), k=10)
    assert torch.equal(idx, widx) and torch.equal(ncand, wncand) and torch.equal(dist.view(torch.int32), wdist.view(torch.int32))
    assert h.probes == "sampled"
    hk, hn = ix.hash_device(q, hash_times=P, probes="ranked")
    assert np.array_equal(hk.cpu().numpy(), keys) and np.array_equal(hn.cpu().numpy(), nkeys)
    assert ix.hash(q[:10], hash_times=P, probes="ranked") == [set(keys[r, :nkeys[r]].tolist()) for r in range(10)]
    ids, counts = ix.query(q, k=10, hash_times=P, probes="ranked")
    wids, wcounts, _, _ = ix.query_with_keys(q, [keys[r, :nkeys[r]].tolist() for r in range(len(keys))], k=10)
    assert ids == wids and counts == wcounts and counts == wncand.cpu().tolist()
    # the sampled mode is what it was: the keyword set to "sampled" is the call without it
    a = ix.query_tensors(q, k=10, hash_times=min(P, 64), seed=4, probes="sampled")
    b = ix.query_tensors(q, k=10, hash_times=min(P, 64), seed=4)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and h.probes == "sampled"


def test_sixteen_ranked_probes_of_a_four_bit_hash_reach_the_whole_corpus():
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    rng = np.random.default_rng(32)
    corpus = dev(rng.standard_normal((4096, 16)).astype(np.float32))
    q = dev(rng.standard_normal((100, 16)).astype(np.float32))
    ix = Indexer(_hasher([16, 32, 4], compat=False), corpus, SIFT.distance, compat=False)
    _, idx, ncand, _ = ix.query_tensors(q, k=10, hash_times=16, probes="ranked")
    assert ncand.cpu().tolist() == [4096] * 100
    assert int(idx.min()) >= 0                                      # every bucket is probed: no list is short
    _, counts = ix.query(q, k=10, hash_times=16, probes="ranked")
    assert counts == [4096] * 100


def test_a_ranked_hasher_takes_no_fused_call_and_no_batch_slot(index_case):
    from nlsh_amd import _capi
    from nlsh_amd.pipeline import QueryPipeline
    ix, h, q, z, code = index_case
    keys, nkeys, _ = rr.table(z, code, 8, 10, _capi.KEY_FULL)
    h.probes = "ranked"
    try:
        assert not ix._fuses(q, 10, _capi.SCAN_BUCKET_TILED)
        with pytest.raises(_capi.NlshHipError) as e:
            QueryPipeline(ix, q, k=10, hash_times=10)
        assert e.value.code == _capi.E_UNSUPPORTED and "ranked" in str(e.value)
        _, idx, ncand, _ = ix.query_tensors(q, k=10, hash_times=10)          # the attribute alone selects the mode
        hk, _ = ix.hash_device(q, hash_times=10, probes="sampled", seed=4)      # ... and the keyword overrides it for a call
        assert h.probes == "ranked"
    finally:
        h.probes = "sampled"
    _, widx, wncand, _ = ix.scan_tensors(q, dev(keys), dev(nkeys), k=10)
    assert torch.equal(idx, widx) and torch.equal(ncand, wncand)
    sk, _ = ix.hash_device(q, hash_times=10, seed=4)
    assert torch.equal(hk, sk)
