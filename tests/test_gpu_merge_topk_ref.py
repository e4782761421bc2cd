"""nlsh_merge_topk against tie_ref.merge_reference, bit for bit: the call is a pure function of its input, so every lane layout of the
narrow kernel (R = 64 // k lists per load from 64 down to 1, lanes past R * k idle), its carry over several rounds, the wide kernels
(2, 3, 4 keys per lane), the count loop past 64 lists, a partial last workgroup and the three forms of the candidate count are checked
on keys chosen for their ties -- not on what a scan happened to produce.  Inputs honour the call's contract: every list ascending and
~0-padded, all real keys of a query distinct (every key has its own id).  Repeated and unsorted lists stay with
test_gpu_wide_k.py::test_merge_topk_with_repeated_lists_stays_inside_its_rows."""
import numpy as np
import pytest
import torch

import tie_ref as T
from helpers import dev

NARROW = [1, 2, 3, 10, 21, 22, 31, 32, 33, 63, 64]
WIDE_G = {2: [1, 3, 4, 7], 3: [1, 2, 5], 4: [1, 2, 5]}                  # keys per lane -> list counts (KPL 2 takes three lists per round)
WIDE = [65, 100, 128, 129, 192, 193, 256]
QS = [1, 4, 5, 9]                                                       # four queries per workgroup; a partial last workgroup
FORMS = ["ncand_in", "stride_k1", "stride_k3", "no_out", "stride_k"]
PAD, BIG_ID = 64, 2 ** 31 - 1
N_PATTERNS = 9


def _list_counts(k):
    if k <= 64:
        R = 64 // k
        return [1, 3 * R, 3 * R + 1, 6 * R + 2]                         # one round, a full one, a second round with one list, three rounds
    return WIDE_G[(k + 63) // 64]


def _pool(rng, pattern, k, G):
    """(distances fp32 of one query's real keys, the lists they may be dealt to); ids are given by the caller."""
    lists = np.arange(G)
    cap = G * k
    f = np.float32
    if pattern == 0:                                                    # one distance word for every key
        d = np.full(min(cap, 3 * k + 5), f(1.5))
    elif pattern == 1:                                                  # three words, the cut strictly inside the second group
        d = np.concatenate([np.full(k // 2, f(0.25)), np.full(k + 3, f(0.5)), np.full(k, f(2.0))])[:cap]
    elif pattern == 2:                                                  # the cut exactly at the second group's end
        d = np.concatenate([np.full(k - k // 3, f(-1.0)), np.full(k // 3, f(0.75)), np.full(k + 1, f(0.75000006))])[:cap]
    elif pattern == 3:                                                  # exactly k keys, two words
        d = np.concatenate([np.full(k - k // 2, f(3.0)), np.full(k // 2, f(7.0))])
    elif pattern == 4:                                                  # distinct floats: negatives, both zeros, infinities, denormals
        special = np.array([-np.inf, np.inf, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -3e-39], f)
        n = min(cap, 2 * k + 8)
        d = np.concatenate([special, rng.standard_normal(max(n - 8, 0)).astype(f) * f(100)])[:n]
        rng.shuffle(d)
    elif pattern == 5:                                                  # distance words 1 ulp apart around the cut, 1-3 keys each
        words = (np.float32(1.0).view(np.uint32) + np.arange(k + 4, dtype=np.uint32)).view(f)
        d = np.repeat(words, rng.integers(1, 4, size=len(words)))[:cap]
    elif pattern == 6:                                                  # fewer than k real keys in total
        d = np.sort(rng.choice(np.array([0.5, 0.5, 1.0, 4.0], f), size=k - 1))
    elif pattern == 7:                                                  # every list all ~0
        d = np.zeros(0, f)
    else:                                                               # an empty list between full ones, heavy ties
        if G >= 3:
            lists = np.delete(lists, 1)
        d = rng.choice(np.array([-2.0, 0.0, 0.125, 0.125, 9.0], f), size=len(lists) * k)
    return d.astype(f), lists


def _make_keys(rng, k, G, Q, stride, shift):
    """keys_in uint64 [G, Q, stride]: columns [0, k) the lists, the rest junk that must not be read (but for column k in the count
    forms, set by the caller)."""
    keys = np.full((G, Q, stride), T.KEY_NONE, dtype=np.uint64)
    keys[:, :, k:] = rng.integers(1, 2 ** 62, size=(G, Q, stride - k), dtype=np.uint64)
    for q in range(Q):
        pattern = (q + shift) % N_PATTERNS
        d, lists = _pool(rng, pattern, k, G)
        n = len(d)
        ids = rng.permutation(np.unique(rng.integers(1, BIG_ID, size=2 * n + 8)))[:n]       # distinct, in [1, 2^31 - 2]
        assert len(ids) == n
        if n >= 2:                                                                          # ids 0 and 2^31 - 1 inside a tie group: that of the median key
            mid = np.nonzero(d == np.sort(d)[min(n - 1, k - 1)])[0]
            ids[mid[0]] = 0
            ids[mid[-1] if len(mid) > 1 else (mid[0] + 1) % n] = BIG_ID
        slots = rng.permutation(len(lists) * k)[:n]                                         # a list never gets more than k keys
        pool = T.make_keys(d, ids)
        for g_pos, g in enumerate(lists):
            mine = np.sort(pool[slots // k == g_pos])
            keys[g, q, :len(mine)] = mine
    return keys


def _call(keys, k, form, rng):
    from nlsh_amd import _capi
    G, Q, stride = keys.shape
    counts = rng.integers(0, 1_000_000, size=(G, Q)).astype(np.int32)
    if form in ("stride_k1", "stride_k3"):
        keys[:, :, k] = counts.astype(np.uint64)
    keys_d = dev(keys.view(np.int64))
    counts_d = dev(counts) if form == "ncand_in" else None
    out_dist = torch.full((Q * k + PAD,), -7.0, dtype=torch.float32, device="cuda")
    out_idx = torch.full((Q * k + PAD,), -7, dtype=torch.int32, device="cuda")
    out_nc = torch.full((Q + PAD,), -7, dtype=torch.int32, device="cuda")
    _capi.check(_capi.lib().nlsh_merge_topk(keys_d.data_ptr(), stride, G, Q, k, None if counts_d is None else counts_d.data_ptr(),
                                            out_dist.data_ptr(), out_idx.data_ptr(), None if form == "no_out" else out_nc.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return counts, out_dist.cpu().numpy(), out_idx.cpu().numpy(), out_nc.cpu().numpy()


def _check(k, G, Q, form, seed):
    rng = np.random.default_rng([k, G, Q, FORMS.index(form), seed])
    stride = {"ncand_in": k + 2, "stride_k1": k + 1, "stride_k3": k + 3, "no_out": k, "stride_k": k}[form]
    keys = _make_keys(rng, k, G, Q, stride, shift=k + G + FORMS.index(form))
    counts, out_dist, out_idx, out_nc = _call(keys, k, form, rng)
    want_dist, want_idx = T.merge_reference(keys, k)
    tag = (k, G, Q, form)
    assert np.all(out_dist[Q * k:] == -7.0) and np.all(out_idx[Q * k:] == -7), tag          # nothing behind the rows
    got_idx, got_bits = out_idx[:Q * k].reshape(Q, k), out_dist[:Q * k].reshape(Q, k).view(np.uint32)
    assert not np.any(got_idx == -7), tag                                                   # every slot written
    assert np.array_equal(got_idx, want_idx), tag
    assert np.array_equal(got_bits, want_dist.view(np.uint32)), tag
    assert np.all(out_nc[Q:] == -7), tag
    if form in ("no_out", "stride_k"):                                                      # no count to take: out_ncand stays untouched
        assert np.all(out_nc[:Q] == -7), tag
    else:
        assert np.array_equal(out_nc[:Q], counts.sum(0, dtype=np.int64).astype(np.int32)), tag


@pytest.mark.gpu
@pytest.mark.parametrize("k", NARROW + WIDE)
def test_merge_topk_is_the_reference_bit_for_bit(k):
    for G in _list_counts(k):
        for Q in QS:
            for form in FORMS:
                _check(k, G, Q, form, seed=0)


@pytest.mark.gpu
def test_merge_topk_with_more_than_64_lists():
    """G = 70 at k = 10: the count loop's second trip (g += 64) and four rounds of the narrow merge."""
    for Q in (5, 9):
        for form in FORMS:
            _check(10, 70, Q, form, seed=1)


def test_the_patterns_are_what_they_claim():
    """The generator, held to its description on the host: ascending ~0-padded lists, distinct keys, and per k every kind of cut."""
    for k in (1, 10, 33, 64, 100, 256):
        G = _list_counts(k)[-1]
        keys = _make_keys(np.random.default_rng(k), k, G, N_PATTERNS, k, shift=0)
        kinds = []
        for q in range(N_PATTERNS):
            lists = keys[:, q, :k]
            real = lists != T.KEY_NONE
            for g in range(G):
                n = int(real[g].sum())
                assert real[g, :n].all() and np.all(np.diff(lists[g, :n].astype(object)) > 0)
            flat = np.sort(lists[real])
            assert len(np.unique(flat & np.uint64(0xFFFFFFFF))) == len(flat)                # every key its own id
            hi = (flat >> np.uint64(32)).astype(np.int64)
            n = len(flat)
            kinds.append("short" if n < k else "exact" if n == k else "inside" if hi[k - 1] == hi[k] else "end")
            if n >= 2:
                low = (flat & np.uint64(0xFFFFFFFF)).astype(np.int64)
                assert 0 in low and BIG_ID in low
        assert kinds[0] == "inside" and kinds[3] == "exact" and kinds[7] == "short" and (kinds[6] == "short")
        assert kinds[2] == "end" and (k < 2 or kinds[1] == "inside") and kinds[5] in ("end", "inside")
