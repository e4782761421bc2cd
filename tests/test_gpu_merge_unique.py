"""nlsh_merge_topk_unique as a pure function, against multi_table_ref.unique_merge_reference on every output word: out_dist bits,
out_idx, out_keys and out_ncand, and nothing written behind them.  Shapes are chosen for where the kernel can go wrong -- every
keys-per-lane class and both sides of each boundary, every lane layout of the narrow class that matters (R = 64 // k lists per
register), one round and several, a partial last workgroup -- and the keys for their repeats: a key is drawn from a UNIVERSE in which
every id has one distance word (the call's precondition) and dealt to any number of the G lists."""
import numpy as np
import pytest
import torch

import multi_table_ref as M
from helpers import dev

T = M.T
KS = [1, 2, 10, 21, 32, 33, 64, 65, 128, 129, 192, 256]
GS = [1, 2, 3, 4, 7, 16]
QS = [1, 4, 5, 9]
FORMS = ["ncand_in", "stride_k1", "stride_k3", "no_out", "stride_k"]
PAD, BIG_ID = 64, 2 ** 31 - 1
PATTERNS = ["disjoint", "identical", "half", "beyond_k", "straddle_k", "one_word", "short", "all_none", "empty_list", "special", "ids"]
SPECIAL = np.array([-np.inf, np.inf, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -3e-39], np.float32)    # test_gpu_merge_topk_ref.py, pattern 4


def _universe(rng, pattern, k, G):
    """(keys uint64 [n] ascending, member bool [G, n]) of one query: list g is the k smallest of keys[member[g]]."""
    f = np.float32
    n = {"disjoint": min(G * k, 2 * k + 5), "identical": k + 3, "short": k - 1, "all_none": 0, "beyond_k": 2 * k, "straddle_k": 2 * k + 2,
         "special": k + 3}.get(pattern, 3 * k)
    if pattern == "one_word":
        d = np.full(n, f(1.5))
    elif pattern == "special":
        d = np.concatenate([SPECIAL, rng.standard_normal(max(n - 8, 0)).astype(f) * f(100)])[:n]
    else:
        d = rng.choice(np.array([-2.0, 0.0, 0.125, 0.5, 0.5, 0.75, 0.75000006, 9.0], f), size=n)                   # heavy ties, words 1 ulp apart
    ids = rng.permutation(np.unique(rng.integers(1, BIG_ID, size=2 * n + 8)))[:n].astype(np.int64)
    assert len(ids) == n
    if n >= 2:
        ids[0], ids[1] = 0, BIG_ID
    if pattern == "ids" and n >= 6:                                                 # at the smallest distance word: no list cuts them off
        ids[2:6] = [-1, -(2 ** 31), -7, -(2 ** 31) + 1]
        d[:6] = f(-2.0)
    keys = np.sort(T.make_keys(d, ids))
    member = rng.random((G, n)) < 0.5
    if pattern == "disjoint":
        slots = rng.permutation(G * k)[:n] // k                                     # a list never gets more than k keys
        member = slots[None, :] == np.arange(G)[:, None]
    elif pattern == "identical":
        member[:] = True
    elif pattern == "beyond_k":                                                     # the union's k best sit in ONE list each, the rest in all
        member[:] = True
        member[:, :k] = rng.integers(0, G, size=k)[None, :] == np.arange(G)[:, None]
    elif pattern == "straddle_k":                                                   # repeats at the union's places k - 1 .. k + 2 only
        member = rng.integers(0, G, size=n)[None, :] == np.arange(G)[:, None]
        member[:, max(k - 2, 0):k + 2] = True
    elif pattern == "empty_list":
        member = rng.random((G, n)) < 0.7
        if G >= 3:
            member[1] = False
    if n and pattern not in ("disjoint", "beyond_k", "straddle_k"):                  # every key of the universe is somewhere
        member[rng.integers(0, G, size=n), np.arange(n)] |= ~member.any(0)
    if pattern == "empty_list" and G >= 3:
        member[1] = False
    return keys, member


def _make_keys(rng, k, G, Q, stride, patterns):
    keys_in = np.full((G, Q, stride), T.KEY_NONE, dtype=np.uint64)
    keys_in[:, :, k:] = rng.integers(1, 2 ** 62, size=(G, Q, stride - k), dtype=np.uint64)  # junk that must not be read (but column k, the count forms)
    for q in range(Q):
        keys, member = _universe(rng, patterns[q % len(patterns)], k, G)
        for g in range(G):
            mine = keys[member[g]][:k]
            keys_in[g, q, :len(mine)] = mine
    return keys_in


def _run(fn_name, keys_in, k, form, rng, with_keys):
    from nlsh_amd import _capi
    G, Q, stride = keys_in.shape
    counts = rng.integers(0, 1_000_000, size=(G, Q)).astype(np.int32)
    if form in ("stride_k1", "stride_k3"):
        keys_in[:, :, k] = counts.astype(np.uint64)
    keys_d = dev(keys_in.view(np.int64))
    counts_d = dev(counts) if form == "ncand_in" else None
    out_dist = torch.full((Q * k + PAD,), -7.0, dtype=torch.float32, device="cuda")
    out_idx = torch.full((Q * k + PAD,), -7, dtype=torch.int32, device="cuda")
    out_keys = torch.full((Q * k + PAD,), -7, dtype=torch.int64, device="cuda")
    out_nc = torch.full((Q + PAD,), -7, dtype=torch.int32, device="cuda")
    args = [keys_d.data_ptr(), stride, G, Q, k, None if counts_d is None else counts_d.data_ptr(), out_dist.data_ptr(), out_idx.data_ptr()]
    if fn_name == "nlsh_merge_topk_unique":
        args.append(out_keys.data_ptr() if with_keys else None)
    args += [None if form == "no_out" else out_nc.data_ptr(), torch.cuda.current_stream().cuda_stream]
    _capi.check(getattr(_capi.lib(), fn_name)(*args))
    torch.cuda.synchronize()
    return counts, out_dist.cpu().numpy(), out_idx.cpu().numpy(), out_keys.cpu().numpy().view(np.uint64), out_nc.cpu().numpy()


def _stride(k, form):
    return {"ncand_in": k + 2, "stride_k1": k + 1, "stride_k3": k + 3, "no_out": k, "stride_k": k}[form]


def _check(k, G, Q, form, with_keys, patterns, seed, also_plain=False):
    rng = np.random.default_rng([k, G, Q, FORMS.index(form), seed])
    keys_in = _make_keys(rng, k, G, Q, _stride(k, form), patterns)
    tag = (k, G, Q, form, with_keys, patterns[0])
    counts, out_dist, out_idx, out_keys, out_nc = _run("nlsh_merge_topk_unique", keys_in, k, form, rng, with_keys)
    want_dist, want_idx, want_keys = M.unique_merge_reference(keys_in, k)
    junk64 = np.array([-7], np.int64).view(np.uint64)[0]
    assert np.all(out_dist[Q * k:] == -7.0) and np.all(out_idx[Q * k:] == -7) and np.all(out_keys[Q * k:] == junk64), tag   # nothing behind the rows
    got_idx, got_bits = out_idx[:Q * k].reshape(Q, k), out_dist[:Q * k].reshape(Q, k).view(np.uint32)
    assert np.array_equal(got_idx, want_idx), tag
    assert np.array_equal(got_bits, want_dist.view(np.uint32)), tag
    if with_keys:
        assert np.array_equal(out_keys[:Q * k].reshape(Q, k), want_keys), tag
    else:
        assert np.all(out_keys == junk64), tag
    assert np.all(out_nc[Q:] == -7), tag
    if form in ("no_out", "stride_k"):                                              # no count to take: out_ncand stays untouched
        assert np.all(out_nc[:Q] == -7), tag
    else:
        assert np.array_equal(out_nc[:Q], counts.sum(0, dtype=np.int64).astype(np.int32)), tag     # the SUM, with multiplicity
    if also_plain:                                                                  # disjoint lists: nlsh_merge_topk's output, word for word
        rng = np.random.default_rng([k, G, Q, FORMS.index(form), seed])
        again = _make_keys(rng, k, G, Q, _stride(k, form), patterns)
        assert np.array_equal(again[:, :, :k], keys_in[:, :, :k])
        _, p_dist, p_idx, _, p_nc = _run("nlsh_merge_topk", again, k, form, rng, False)
        assert np.array_equal(p_dist.view(np.uint32), out_dist.view(np.uint32)) and np.array_equal(p_idx, out_idx) and np.array_equal(p_nc, out_nc), tag


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_merge_topk_unique_is_the_reference_on_every_word(k):
    """Every (G, Q) of the grid; the count form and out_keys null / non-null cycle so that each G sees every form and both; the queries of a
    call cycle through the patterns from a moving start, and one call per G of len(PATTERNS) queries holds them all."""
    i = 0
    for G in GS:
        for Q in QS + [len(PATTERNS)]:
            start = i % len(PATTERNS)
            _check(k, G, Q, FORMS[i % len(FORMS)], with_keys=bool((i // len(FORMS) + i) % 2), patterns=PATTERNS[start:] + PATTERNS[:start], seed=0)
            i += 1


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_on_disjoint_lists_it_is_nlsh_merge_topk_word_for_word(k):
    for j, G in enumerate(GS):
        _check(k, G, 5, FORMS[j % 3], with_keys=True, patterns=["disjoint"], seed=1, also_plain=True)


@pytest.mark.gpu
def test_every_form_with_and_without_keys_at_one_shape_per_class():
    for k, G in ((10, 7), (64, 16), (100, 4), (129, 3), (256, 16)):
        for form in FORMS:
            for with_keys in (False, True):
                _check(k, G, 9, form, with_keys, PATTERNS, seed=2)


def test_the_patterns_are_what_they_claim():
    """The generator held to its description on the host: ascending ~0-padded lists, distinct within a list, one distance word per id
    across lists (the precondition), and per pattern the repeats it names."""
    for k in (1, 10, 33, 64, 100, 256):
        for G in (1, 3, 16):
            rng = np.random.default_rng([k, G])
            keys_in = _make_keys(rng, k, G, len(PATTERNS), k, PATTERNS)
            for q, pattern in enumerate(PATTERNS):
                lists = keys_in[:, q, :k]
                real = lists != T.KEY_NONE
                for g in range(G):
                    n = int(real[g].sum())
                    assert real[g, :n].all() and np.all(np.diff(lists[g, :n].astype(object)) > 0), (k, G, pattern)
                flat = lists[real]
                uniq = np.unique(flat)
                assert len(np.unique(uniq & M.LOW32)) == len(uniq), (k, G, pattern)              # one key, hence one distance word, per id
                repeats = len(flat) - len(uniq)
                first = uniq[:k]
                mult = np.array([int((flat == u).sum()) for u in uniq])
                if pattern == "disjoint":
                    assert repeats == 0 and len(uniq) >= min(k, 2)
                elif pattern == "identical":
                    assert len(uniq) == k and repeats == (G - 1) * k
                elif pattern == "beyond_k" and G > 1:
                    assert np.all(mult[:k] == 1) and len(uniq) > k and mult[k:].max() > 1
                elif pattern == "straddle_k" and G > 1 and k >= 2:
                    assert mult[k - 1] == G and mult[k] == G and np.all(mult[:k - 2] == 1)
                elif pattern == "one_word":
                    assert len(np.unique(uniq >> np.uint64(32))) == 1 and (G == 1 or repeats > 0 or k == 1)
                elif pattern == "short":
                    assert len(uniq) == k - 1
                elif pattern == "all_none":
                    assert len(flat) == 0
                elif pattern == "empty_list" and G >= 3:
                    assert not real[1].any() and real[0].any() and real[2].any()
                elif pattern == "special":
                    have = T.float_from_mono((uniq >> np.uint64(32)).astype(np.uint32)).view(np.uint32)
                    assert k < 10 or (SPECIAL.view(np.uint32)[0] in have and np.isin(SPECIAL.view(np.uint32), have).sum() >= 6)
                elif pattern == "ids" and k >= 6:
                    low = (uniq & M.LOW32).astype(np.uint32).view(np.int32)
                    assert {0, BIG_ID, -1, -(2 ** 31)} <= set(low.tolist())
                assert len(first) <= k
