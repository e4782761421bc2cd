"""The candidate budget of ranked probes on the GPU: `nlsh_probe_ranked_budget` on injected pre-activations and synthetic CSR arrays,
through the hasher and through the `Indexer` (`candidate_budget=`), each against the numpy reference of tests/ranked_budget_ref.py.
Every row is compared and nothing has a tolerance: keys, counts, fp32 cost bits and candidate counts are pinned word for word."""
import functools

import numpy as np
import pytest
import torch

import ranked_budget_ref as rbr
import ranked_ref as rr
from helpers import dev, make_hashing

pytestmark = pytest.mark.gpu

P_ALL = (1, 2, 10, 64, 65, 128)        # 65 crosses one kept slot per lane, 128 fills both register sets
N_ROWS = 203                           # not a multiple of the 4 rows per workgroup


def budget_probe(z, codes, H, P, key_mode, uniq, offsets, budget, n_multi_rows=None, want_cost=True, want_ncand=True):
    """One `nlsh_probe_ranked_budget` call on device tensors (`uniq` None = an empty index) -> (keys, nkeys, cost bits, ncand)."""
    from nlsh_amd import _capi
    n = z.shape[0]
    keys = torch.full((n, P), -7, dtype=torch.int32, device=z.device)
    nkeys = torch.full((n,), -7, dtype=torch.int32, device=z.device)
    cost = torch.full((n, P), -7.0, dtype=torch.float32, device=z.device) if want_cost else None
    ncand = torch.full((n,), -7, dtype=torch.int32, device=z.device) if want_ncand else None
    _capi.check(_capi.lib().nlsh_probe_ranked_budget(
        _capi.ptr(z), z.stride(0), _capi.ptr(codes), n, H, key_mode, P, n if n_multi_rows is None else n_multi_rows,
        _capi.ptr(uniq), _capi.ptr(offsets), 0 if uniq is None else uniq.shape[0], budget, _capi.ptr(keys), _capi.ptr(nkeys),
        _capi.ptr(cost), _capi.ptr(ncand), torch.cuda.current_stream(z.device).cuda_stream))
    torch.cuda.synchronize()
    return (keys.cpu().numpy(), nkeys.cpu().numpy(), None if cost is None else cost.cpu().numpy().view(np.uint32),
            None if ncand is None else ncand.cpu().numpy())


def plain_probe(z, codes, H, P, key_mode, n_multi_rows=None):
    """`nlsh_probe_ranked`, the unbudgeted call -> (keys, nkeys, cost bits)."""
    from nlsh_amd import _capi
    n = z.shape[0]
    keys = torch.full((n, P), -7, dtype=torch.int32, device=z.device)
    nkeys = torch.full((n,), -7, dtype=torch.int32, device=z.device)
    cost = torch.full((n, P), -7.0, dtype=torch.float32, device=z.device)
    _capi.check(_capi.lib().nlsh_probe_ranked(_capi.ptr(z), z.stride(0), _capi.ptr(codes), n, H, key_mode, P,
                                              n if n_multi_rows is None else n_multi_rows, _capi.ptr(keys), _capi.ptr(nkeys),
                                              _capi.ptr(cost), torch.cuda.current_stream(z.device).cuda_stream))
    torch.cuda.synchronize()
    return keys.cpu().numpy(), nkeys.cpu().numpy(), cost.cpu().numpy().view(np.uint32)


def assert_table(got, want, what):
    for name, g, w in zip(("keys", "nkeys", "cost", "ncand"), got, want):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())


def mixed_rows(n, H, seed):
    """Thirds of `rr.random_rows`, `rr.tie_rows` and `rr.absorbing_rows`, interleaved."""
    z = rr.random_rows(n, H, seed)
    z[1::3] = rr.tie_rows(len(z[1::3]), H, seed + 1)
    z[2::3] = rr.absorbing_rows(len(z[2::3]), H, seed + 2)
    return z


@functools.lru_cache(maxsize=None)
def rows_case(H, key_mode):
    """(z, codes, {P: unbudgeted reference table}) of the rows every kernel test of one (H, key_mode) shares; computed once."""
    z = mixed_rows(N_ROWS, H, seed=10 * H + key_mode)
    codes = rr.hard_codes(z, H)
    codes[::7] = np.random.default_rng(H).integers(0, 1 << H, size=len(codes[::7]), dtype=np.uint64).astype(np.uint32)   # any code, not only z's own
    return z, codes, {}


def full_table(H, key_mode, P):
    z, codes, tables = rows_case(H, key_mode)
    if P not in tables:
        tables[P] = rr.table(z, codes, H, P, key_mode)
    return tables[P]


def csr_for(H, key_mode, nb, seed, extremes=False):
    """Synthetic CSR arrays of `nb` buckets for the rows of `rows_case`: up to half of the keys are sampled from the keys the rows probe
    (so probes find buckets, but at most half of them do), the rest from the whole code space (most of those are never asked for);
    heavy-tailed sizes."""
    keys, nkeys, _ = full_table(H, key_mode, 64)
    rng = np.random.default_rng(seed)
    probed = np.unique(keys[np.arange(64)[None, :] < nkeys[:, None]])
    take = rng.permutation(probed)[:min((nb + 1) // 2, len(probed) // 2)]
    include = list(take) + ([-2 ** 31, 2 ** 31 - 1] if extremes else [])
    uniq = rbr.sampled_uniq_keys(nb, H, key_mode, seed, include=include[:nb])
    if not extremes and nb > 2:                 # some probed keys lie below the first and above the last bucket
        lo, hi = int(probed.min()), int(probed.max())
        inner = set(uniq[(uniq > lo) & (uniq < hi)].tolist())
        while len(inner) < nb:
            inner.add(int(rng.integers(lo + 1, hi)))
        uniq = np.array(sorted(inner), dtype=np.int32)
    return uniq, rbr.heavy_tailed_csr(uniq, seed + 1)


def stop_shares(full, uniq, offsets, budget):
    """Of the reference's rows at this budget: (share that stops before its nk, share that reaches nk below the budget)."""
    _, nkeys, _, ncand = rbr.cut(*full, uniq, offsets, budget)
    return float(np.mean(nkeys < full[1])), float(np.mean((nkeys == full[1]) & (ncand < budget)))


def check_budgets(H, key_mode, P, uniq, offsets, what, mixed=False):
    """Budgets 1, INT32_MAX and the median of cum / 2 for one (rows, P, index): kernel == reference, INT32_MAX == the unbudgeted kernel."""
    z, codes, _ = rows_case(H, key_mode)
    zd, cd = dev(z), dev(codes.view(np.int32))
    ud, od = (None, None) if len(uniq) == 0 else (dev(uniq), dev(offsets))
    full = full_table(H, key_mode, P)
    median = rbr.median_budget(full[0], full[1], uniq, offsets)
    for budget in (1, rbr.INT32_MAX, median):
        want = rbr.cut(*full, uniq, offsets, budget)
        assert_table(budget_probe(zd, cd, H, P, key_mode, ud, od, budget), want, (what, P, budget))
        if budget == rbr.INT32_MAX:
            assert_table(plain_probe(zd, cd, H, P, key_mode), want[:3], (what, P, "plain"))
            assert_table(want[:3], full, (what, P, "prefix of itself"))
    if mixed:       # neither a never-stopping nor an always-stopping kernel passes: asserted on the reference
        early, short = stop_shares(full, uniq, offsets, median)
        assert early >= 0.10 and short >= 0.10, (what, P, median, early, short)


# ---------------------------------------------------------------------------- the kernel on injected z
@pytest.mark.parametrize("key_mode", [rr.KEY_REF_INT16, rr.KEY_FULL])
@pytest.mark.parametrize("H", [1, 4, 8, 16, 17, 24, 32])
def test_injected_rows_match_the_reference(H, key_mode):
    bits = min(H, 16) if key_mode == rr.KEY_REF_INT16 else H
    uniq, offsets = csr_for(H, key_mode, min(3000, max(1, (1 << bits) * 2 // 3)), seed=H)
    for P in P_ALL:
        # (where P probes are a large share of the 2^bits codes every row sees much the same buckets, and the shares are not asked for)
        check_budgets(H, key_mode, P, uniq, offsets, (H, key_mode), mixed=P >= 10 and (1 << bits) >= 8 * P)
    # fewer rows than a workgroup, and the single-probe tail
    z, codes, _ = rows_case(H, key_mode)
    median = rbr.median_budget(*full_table(H, key_mode, 10)[:2], uniq, offsets)
    ud, od = dev(uniq), dev(offsets)
    for n in (1, 5, N_ROWS):
        zd, cd = dev(z[:n]), dev(codes[:n].view(np.int32))
        for n_multi in (0, n - 2, n):
            for P in (10, 65):
                want = rbr.table(z[:n], codes[:n], H, P, key_mode, uniq, offsets, median, n_multi_rows=n_multi) if n < N_ROWS else None
                if want is None:                  # the shared table, the rows past n_multi cut down to their hard key
                    full = full_table(H, key_mode, P)
                    one = rr.table(z[n_multi:], codes[n_multi:], H, 1, key_mode)
                    keys, nkeys, cost = (a.copy() for a in full)
                    keys[n_multi:], cost[n_multi:], nkeys[n_multi:] = 0, rr.INF_BITS, 1
                    keys[n_multi:, :1], cost[n_multi:, :1] = one[0], one[2]
                    want = rbr.cut(keys, nkeys, cost, uniq, offsets, median)
                got = budget_probe(zd, cd, H, P, key_mode, ud, od, median, n_multi_rows=n_multi)
                assert_table(got, want, (H, key_mode, n, n_multi, P))
                assert (got[1][max(n_multi, 0):] == 1).all()


# ---------------------------------------------------------------------------- CSR arrays at the search's edges
@pytest.mark.parametrize("nb,H", [(0, 8), (1, 4), (2, 4), (63, 8), (64, 8), (65, 8), (4096, 16), (4097, 16), (70001, 18)])
def test_bucket_counts_at_the_edges_of_the_64_way_search(nb, H):
    """0 buckets (no search), 1, 2, and one either side of every size at which the search takes another round (64, 64^2); 70,001
    takes three.  Full-width keys."""
    uniq, offsets = csr_for(H, rr.KEY_FULL, nb, seed=nb) if nb else (np.zeros((0,), np.int32), np.zeros((1,), np.int32))
    assert len(uniq) == nb and (np.diff(uniq.astype(np.int64)) > 0).all()
    for P in (10, 128):
        check_budgets(H, rr.KEY_FULL, P, uniq, offsets, ("nb", nb), mixed=nb >= 63)
    if nb > 2:
        sizes = np.diff(offsets)
        assert (sizes == 0).any() and (sizes == 1).sum() > nb // 3 and (nb < 4096 or (sizes >= 1000).any())     # heavy-tailed, zero-length buckets
        keys, nkeys, _ = full_table(H, rr.KEY_FULL, 128)
        probed = keys[np.arange(128)[None, :] < nkeys[:, None]]
        assert (probed < uniq[0]).any() and (probed > uniq[-1]).any()                # keys below the first and above the last entry
        assert np.mean(rbr.sizes_of(probed, uniq, offsets) == 0) > 0.5                   # most probes find no bucket


@pytest.mark.parametrize("nb", [65, 4097, 70001])
def test_negative_keys_are_searched_in_signed_order(nb):
    """Full-width keys of a 32-bit hash: half of them negative, INT32_MIN and INT32_MAX among the buckets."""
    H = 32
    uniq, offsets = csr_for(H, rr.KEY_FULL, nb, seed=nb + 5, extremes=True)
    assert len(uniq) == nb and uniq[0] == -2 ** 31 and uniq[-1] == 2 ** 31 - 1 and (np.diff(uniq.astype(np.int64)) > 0).all()
    assert 0.3 < np.mean(uniq < 0) < 0.7
    for P in (10, 65):
        check_budgets(H, rr.KEY_FULL, P, uniq, offsets, ("signed", nb), mixed=nb >= 4097)     # (65 buckets of 2^32 keys: few rows meet any)
    # the extreme buckets themselves are asked for: rows whose hard codes are 0x80000000 and 0x7FFFFFFF
    z = rr.random_rows(6, H, seed=1)
    codes = np.array([0x80000000, 0x7FFFFFFF] * 3, dtype=np.uint32)
    for budget in (1, 50, rbr.INT32_MAX):
        want = rbr.table(z, codes, H, 10, rr.KEY_FULL, uniq, offsets, budget)
        assert_table(budget_probe(dev(z), dev(codes.view(np.int32)), H, 10, rr.KEY_FULL, dev(uniq), dev(offsets), budget), want, ("extremes", budget))
    sizes = rbr.sizes_of(codes.view(np.int32), uniq, offsets)
    assert np.array_equal(rbr.table(z, codes, H, 1, rr.KEY_FULL, uniq, offsets, 1)[3], sizes)


# ---------------------------------------------------------------------------- colliding int16 keys
@pytest.mark.parametrize("H", [24, 32])
def test_a_colliding_int16_key_takes_no_slot_and_is_counted_once(H):
    """The two cheapest flips sit in code bits >= 16, which a 16-bit key does not see: the first four pops are one key, and later
    pops that flip another high bit repeat earlier keys too.  Every 16-bit
    key has a bucket of 10 rows and the budget is 25, so a row stops at its THIRD distinct key; counting a repeated key again would
    stop it at the third pop, with one key."""
    n, hi = 41, 2
    z = rr.random_rows(n, H, seed=H) + np.float32(3.0) * np.sign(rr.random_rows(n, H, seed=H))
    z[:, :hi] = (rr.random_rows(n, hi, seed=H + 1) * np.float32(1e-3))          # hasher bits 0 and 1 are code bits H-1 and H-2: the first four pops
    z[::5, :hi] = rr.tie_rows(len(z[::5]), hi, seed=H + 2) * np.float32(1e-3)
    codes = rr.hard_codes(z, H)
    uniq = np.arange(-32768, 32768, dtype=np.int32)
    offsets = (np.arange(65537, dtype=np.int64) * 10).astype(np.int32)
    zd, cd, ud, od = dev(z), dev(codes.view(np.int32)), dev(uniq), dev(offsets)
    for P in (16, 65, 128):
        full = rr.table(z, codes, H, P, rr.KEY_REF_INT16)
        raw = rr.table(z, codes, H, 3, rr.KEY_FULL)[0]                         # the first three pops as full-width keys
        assert (raw.astype(np.int16) == raw[:, :1].astype(np.int16)).all()      # ... collide with the hard key
        want = rbr.cut(*full, uniq, offsets, 25)
        reach = full[1] >= 3
        assert reach.any() and (want[1][reach] == 3).all() and (want[3][reach] == 30).all()
        assert_table(budget_probe(zd, cd, H, P, rr.KEY_REF_INT16, ud, od, 25), want, (H, P, 25))
        for budget in (1, 10, 11, rbr.INT32_MAX):
            assert_table(budget_probe(zd, cd, H, P, rr.KEY_REF_INT16, ud, od, budget), rbr.cut(*full, uniq, offsets, budget), (H, P, budget))
        assert_table(plain_probe(zd, cd, H, P, rr.KEY_REF_INT16), full, (H, P, "plain"))
    # heavy-tailed sizes on the same rows
    offsets = rbr.heavy_tailed_csr(uniq, seed=H)
    full = rr.table(z, codes, H, 128, rr.KEY_REF_INT16)
    for budget in (1, rbr.median_budget(full[0], full[1], uniq, offsets), rbr.INT32_MAX):
        assert_table(budget_probe(zd, cd, H, 128, rr.KEY_REF_INT16, ud, dev(offsets), budget), rbr.cut(*full, uniq, offsets, budget), (H, "tail", budget))


# ---------------------------------------------------------------------------- strided z, optional outputs
def test_strided_z_and_optional_outputs():
    H, P, n = 17, 65, 23
    wide = np.full((n, 40), np.nan, dtype=np.float32)         # the columns past H are never read
    wide[:, :H] = mixed_rows(n, H, seed=11)
    codes = rr.hard_codes(wide[:, :H], H)
    full = rr.table(wide[:, :H], codes, H, P, rr.KEY_FULL)
    valid = np.arange(P)[None, :] < full[1][:, None]
    uniq = rbr.sampled_uniq_keys(2000, H, rr.KEY_FULL, seed=3, include=np.random.default_rng(3).permutation(np.unique(full[0][valid]))[:700])
    offsets = rbr.heavy_tailed_csr(uniq, seed=4)
    budget = rbr.median_budget(full[0], full[1], uniq, offsets)
    want = rbr.cut(*full, uniq, offsets, budget)
    assert (want[1] < full[1]).any() and (want[1] == full[1]).any()
    wd, cd, ud, od = dev(wide), dev(codes.view(np.int32)), dev(uniq), dev(offsets)
    view = wd[:, :H]
    assert view.stride(0) == 40
    assert_table(budget_probe(view, cd, H, P, rr.KEY_FULL, ud, od, budget), want, "strided")
    assert_table(budget_probe(view.contiguous(), cd, H, P, rr.KEY_FULL, ud, od, budget), want, "contiguous copy")
    for a, b in ((0, 1), (3, 10), (9, 23)):                     # a row's result does not depend on its batch
        assert_table(budget_probe(view[a:b], cd[a:b], H, P, rr.KEY_FULL, ud, od, budget), tuple(t[a:b] for t in want), (a, b))
    keys, nkeys, cost, ncand = budget_probe(view, cd, H, P, rr.KEY_FULL, ud, od, budget, want_cost=False, want_ncand=False)
    assert cost is None and ncand is None and np.array_equal(keys, want[0]) and np.array_equal(nkeys, want[1])


# ---------------------------------------------------------------------------- through the hasher and the Indexer
N, D, HASH, Q, K, CAP = 20000, 32, 12, 300, 10, 32
BUDGETS = (1, 200, 10 ** 9)


@pytest.fixture(scope="module", params=[64, 640], ids=["lds", "streamed"])
def index_case(request):
    """(indexer, hasher, queries, z, code, CSR arrays on the host) of one encoder form; z and the hard codes are the encoder's own."""
    from nlsh_amd import synth
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    dims = [D, request.param, HASH]
    Ws, bs = synth.make_weights(dims, seed=3, gain=3.0)
    h = make_hashing(D, dims[1:-1], HASH, Ws, bs, compat=False)
    assert h.streamed() == (request.param > 632)
    rng = np.random.default_rng(41)
    corpus = dev(rng.standard_normal((N, D)).astype(np.float32))
    q = dev(rng.standard_normal((Q, D)).astype(np.float32))
    ix = Indexer(h, corpus, SIFT.distance, compat=False)
    z, _, code = h.forward_device(q)
    torch.cuda.synchronize()
    return ix, h, q, z.cpu().numpy(), code.cpu().numpy().view(np.uint32), ix.uniq_keys.cpu().numpy(), ix.offsets.cpu().numpy()


@pytest.mark.parametrize("budget", BUDGETS)
def test_the_indexer_probes_to_the_budget(index_case, budget):
    from nlsh_amd import _capi
    ix, h, q, z, code, uniq, offsets = index_case
    full = rr.table(z, code, HASH, CAP, _capi.KEY_FULL)
    keys, nkeys, _, cum = rbr.cut(*full, uniq, offsets, budget)
    calls = repr(h._calls)
    hk, hn = ix.hash_device(q, hash_times=CAP, probes="ranked", candidate_budget=budget)
    assert np.array_equal(hk.cpu().numpy(), keys) and np.array_equal(hn.cpu().numpy(), nkeys)
    got = budget_probe(dev(z), dev(code.view(np.int32)), HASH, CAP, _capi.KEY_FULL, ix.uniq_keys, ix.offsets, min(budget, rbr.INT32_MAX))
    assert np.array_equal(got[3], cum)                                              # ncand_out
    dist, idx, ncand, _ = ix.query_tensors(q, k=K, hash_times=CAP, probes="ranked", candidate_budget=budget)
    nc = ncand.cpu().numpy()
    assert np.array_equal(nc, cum) and np.array_equal(nc, got[3])
    assert ((nc >= budget) | (nkeys == full[1])).all()                              # the budget is met, or the cap / the code space ended the row
    last = rbr.sizes_of(keys[np.arange(Q), nkeys - 1], uniq, offsets)
    assert (((nc - last) < budget) | (nkeys == 1)).all()                            # ... and no key was probed after it was met
    wdist, widx, wncand, _ = ix.scan_tensors(q, dev(keys), dev(nkeys), k=K)
    assert torch.equal(idx, widx) and torch.equal(ncand, wncand) and torch.equal(dist.view(torch.int32), wdist.view(torch.int32))
    ids, counts = ix.query(q, k=K, hash_times=CAP, probes="ranked", candidate_budget=budget)
    assert counts == nc.tolist() and ids == [[v for v in row if v >= 0] for row in widx.cpu().tolist()]
    assert ix.hash(q[:40], hash_times=CAP, probes="ranked", candidate_budget=budget) == \
        [set((keys[r, :nkeys[r]].astype(np.int64) & 0xFFFFFFFF).tolist()) for r in range(40)]
    assert h.probes == "sampled" and repr(h._calls) == calls                        # no seed was drawn, the hasher is as it was
    if budget == 200:
        assert (nkeys < full[1]).mean() > 0.1 and (nkeys > 1).mean() > 0.1          # the budget does cut, and not at the hard key alone
    if budget == 10 ** 9:                                                           # never met: the plain ranked call, exactly
        pk, pn = ix.hash_device(q, hash_times=CAP, probes="ranked")
        assert torch.equal(hk, pk) and torch.equal(hn, pn)
        pdist, pidx, pncand, _ = ix.query_tensors(q, k=K, hash_times=CAP, probes="ranked")
        assert torch.equal(idx, pidx) and torch.equal(ncand, pncand) and torch.equal(dist.view(torch.int32), pdist.view(torch.int32))
        assert ix.query(q, k=K, hash_times=CAP, probes="ranked") == (ids, counts)


def test_a_ranked_hasher_needs_no_keyword_and_a_cap_above_64_is_scanned_in_slices(index_case):
    from nlsh_amd import _capi
    ix, h, q, z, code, uniq, offsets = index_case
    cap, budget = 100, 600
    keys, nkeys, _, cum = rbr.table(z, code, HASH, cap, _capi.KEY_FULL, uniq, offsets, budget)
    assert (nkeys > 64).any()
    h.probes = "ranked"
    try:
        dist, idx, ncand, _ = ix.query_tensors(q, k=K, hash_times=cap, candidate_budget=budget)
        hk, hn = ix.hash_device(q, hash_times=cap, candidate_budget=budget)
        with pytest.raises(ValueError, match="ranked"):
            ix.query_tensors(q, k=K, hash_times=cap, candidate_budget=budget, probes="sampled")
    finally:
        h.probes = "sampled"
    assert np.array_equal(hk.cpu().numpy(), keys) and np.array_equal(hn.cpu().numpy(), nkeys) and np.array_equal(ncand.cpu().numpy(), cum)
    wdist, widx, wncand, _ = ix.scan_tensors(q, dev(keys), dev(nkeys), k=K)
    assert torch.equal(idx, widx) and torch.equal(ncand, wncand) and torch.equal(dist.view(torch.int32), wdist.view(torch.int32))
    with pytest.raises(_capi.NlshHipError) as e:
        ix.hash_device(q, hash_times=_capi.MAX_ENCODE_PROBES + 1, probes="ranked", candidate_budget=budget)
    assert e.value.code == _capi.E_UNSUPPORTED


def test_the_trailing_batch_of_a_compat_indexer_gets_one_key():
    from nlsh_amd import _capi, synth
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    dims = [D, 64, HASH]
    Ws, bs = synth.make_weights(dims, seed=3, gain=3.0)
    h = make_hashing(D, dims[1:-1], HASH, Ws, bs, compat=True)
    rng = np.random.default_rng(42)
    ix = Indexer(h, dev(rng.standard_normal((N, D)).astype(np.float32)), SIFT.distance, compat=True)
    q = dev(rng.standard_normal((Q, D)).astype(np.float32))
    z, _, code = h.forward_device(q)
    z, code, uniq, offsets = z.cpu().numpy(), code.cpu().numpy().view(np.uint32), ix.uniq_keys.cpu().numpy(), ix.offsets.cpu().numpy()
    # batches of 128: rows 0..255 are multi-probe, the trailing 44 rows keep their hard key (the reference's rule F6)
    want = rbr.table(z, code, HASH, CAP, _capi.KEY_REF_INT16, uniq, offsets, 200, n_multi_rows=256)
    hk, hn = ix.hash_device(q, batch_size=128, hash_times=CAP, probes="ranked", candidate_budget=200)
    assert np.array_equal(hk.cpu().numpy(), want[0]) and np.array_equal(hn.cpu().numpy(), want[1])
    assert (want[1][256:] == 1).all() and (want[1][:256] > 1).any()
    assert ix.hash(q, batch_size=128, hash_times=CAP, probes="ranked", candidate_budget=200) == [set(want[0][r, :want[1][r]].tolist()) for r in range(Q)]
    # a query batch shorter than the default 4096-row hash batch is all trailing: every row probes its hard bucket alone
    _, _, ncand, _ = ix.query_tensors(q, k=K, hash_times=CAP, probes="ranked", candidate_budget=200)
    assert np.array_equal(ncand.cpu().numpy(), rbr.sizes_of(code.view(np.int32), uniq, offsets))
    ids, counts = ix.query(q, k=K, hash_times=CAP, probes="ranked", candidate_budget=200)
    assert counts == ncand.cpu().tolist() and ix.query(q, k=K, hash_times=1) == (ids, counts)


def test_a_batchnorm_encoder_in_train_mode_is_refused_as_for_ranked():
    from nlsh_amd import _capi
    from nlsh_amd.data import SIFT
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.hashings import MultivariateBernoulli
    from nlsh_amd.indexer import Indexer
    h = MultivariateBernoulli(MultiLayerRelu(8, [16], with_batchnorm=True), 6, None, compat=False)
    h.train_mode(False)
    rng = np.random.default_rng(2)
    ix = Indexer(h, dev(rng.standard_normal((500, 8)).astype(np.float32)), SIFT.distance, compat=False)
    x = dev(rng.standard_normal((32, 8)).astype(np.float32))
    assert ix.hash_device(x, hash_times=4, probes="ranked", candidate_budget=50)[0].shape == (32, 4)
    h.train_mode(True)
    with pytest.raises(_capi.NlshHipError) as e:
        ix.hash_device(x, hash_times=4, probes="ranked", candidate_budget=50)
    assert e.value.code == _capi.E_UNSUPPORTED and "eval mode" in str(e.value)
