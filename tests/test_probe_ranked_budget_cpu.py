"""The candidate budget of ranked probes, the parts that need no device: the numpy reference (tests/ranked_budget_ref.py) against a
brute-force restatement, `nlsh_probe_ranked_budget`'s host-side refusals through the C ABI, and the facade's ValueErrors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ranked_budget_ref as rbr
import ranked_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {"random": rr.random_rows, "ties": rr.tie_rows, "absorbing": rr.absorbing_rows}


@pytest.fixture(scope="module")
def L():
    from nlsh_amd import _capi
    return _capi.lib()


# ---------------------------------------------------------------------------- the reference
def restated(row_keys, row_costs, size_of, budget, P):
    """The definition once more, in plain Python on one row's unbudgeted (keys, costs): walk the keys, stop after the first that
    brings the sum of its buckets to the budget."""
    kept, cum = 0, 0
    for key in row_keys:
        kept, cum = kept + 1, cum + size_of.get(key, 0)
        if cum >= budget:
            break
    return (row_keys[:kept] + [0] * (P - kept), kept, row_costs[:kept] + [rr.INF_BITS] * (P - kept), cum)


def check_against_restatement(z, codes, H, P, key_mode, uniq, offsets, budgets, fn):
    size_of = {int(k): int(offsets[b + 1] - offsets[b]) for b, k in enumerate(uniq)}
    stopped = 0
    for budget in budgets:
        keys, nkeys, cost, ncand = rbr.table(z, codes, H, P, key_mode, uniq, offsets, budget)
        for r in range(len(codes)):
            rk, rc = fn(z[r], int(codes[r]), H, P, key_mode)
            wk, wn, wc, wcum = restated(rk, rc, size_of, budget, P)
            assert (keys[r].tolist(), int(nkeys[r]), cost[r].tolist(), int(ncand[r])) == (wk, wn, wc, wcum), (H, P, key_mode, budget, r)
            stopped += wn < len(rk)
    return stopped


@pytest.mark.parametrize("kind", sorted(ROWS))
@pytest.mark.parametrize("H", [1, 2, 5, 8, 10])
def test_the_reference_equals_the_brute_force_enumeration_plus_the_cut(kind, H):
    z = ROWS[kind](6, H, seed=50 * H + len(kind))
    codes = rr.hard_codes(z, H)
    stopped = 0
    for key_mode in (rr.KEY_REF_INT16, rr.KEY_FULL):
        uniq = rbr.sampled_uniq_keys(max(1, (1 << H) * 2 // 3), H, key_mode, seed=H)
        offsets = rbr.heavy_tailed_csr(uniq, seed=H + 1)
        for P in (1, 7, 64, 128):
            stopped += check_against_restatement(z, codes, H, P, key_mode, uniq, offsets, (1, 3, 40, 5000, rbr.INT32_MAX), rr.brute)
    assert stopped or H == 1                                        # some rows do stop before their last key


def test_the_reference_counts_a_colliding_int16_key_once():
    """H > 16 with int16 keys (`best_first`: 2^H subsets cannot be enumerated): the cheapest flips sit in the bits a 16-bit key does not
    see, so the first pops repeat the hard key; they take no slot and their bucket is counted once."""
    H, P = 20, 32
    z = np.full((3, H), 5.0, dtype=np.float32)
    z[:, :4] = [0.1, -0.2, 0.3, -0.4]
    z[:, 4:] += np.random.default_rng(4).random((3, H - 4)).astype(np.float32)
    codes = rr.hard_codes(z, H)
    uniq = np.array(sorted({rr.key_of(int(c), rr.KEY_REF_INT16) for c in codes}), dtype=np.int32)
    offsets = (np.arange(len(uniq) + 1) * 10).astype(np.int32)      # the hard bucket holds 10 rows, every other key none
    stopped = check_against_restatement(z, codes, H, P, rr.KEY_REF_INT16, uniq, offsets, (10, 11, 20), rr.best_first)
    keys, nkeys, _, ncand = rbr.table(z, codes, H, P, rr.KEY_REF_INT16, uniq, offsets, 20)
    full = rr.table(z, codes, H, P, rr.KEY_REF_INT16)
    assert np.array_equal(nkeys, full[1]) and (nkeys < P).all() and ncand.tolist() == [10] * 3     # a duplicate counted twice would reach 20
    assert rbr.table(z, codes, H, P, rr.KEY_REF_INT16, uniq, offsets, 10)[1].tolist() == [1] * 3 and stopped


def test_int32_max_is_the_unbudgeted_table_and_an_empty_index_never_stops():
    H, P = 9, 64
    z = rr.random_rows(7, H, seed=2)
    codes = rr.hard_codes(z, H)
    uniq = rbr.sampled_uniq_keys(300, H, rr.KEY_FULL, seed=1)
    offsets = rbr.heavy_tailed_csr(uniq, seed=2)
    want = rr.table(z, codes, H, P, rr.KEY_FULL, n_multi_rows=5)
    got = rbr.table(z, codes, H, P, rr.KEY_FULL, uniq, offsets, rbr.INT32_MAX, n_multi_rows=5)
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], want))
    assert np.array_equal(got[3], rbr.unbudgeted_cum(want[0], want[1], uniq, offsets))
    none = rbr.table(z, codes, H, P, rr.KEY_FULL, np.zeros((0,), np.int32), np.zeros((1,), np.int32), 1, n_multi_rows=5)
    assert all(np.array_equal(g, w) for g, w in zip(none[:3], want)) and not none[3].any()
    one = rbr.table(z, codes, H, P, rr.KEY_FULL, uniq, offsets, 1)
    assert (one[1] >= 1).all() and np.array_equal(one[0][:, 0], codes.view(np.int32))        # slot 0 is kept whatever it holds


# ---------------------------------------------------------------------------- the C ABI's host-side checks
def _call(L, z=True, code=True, keys=True, nkeys=True, uniq=True, offsets=True, n=8, H=16, z_stride=None, key_mode=1, P=10, n_multi=None,
          n_buckets=5, budget=100):
    """nlsh_probe_ranked_budget with pointers into a small host buffer: every call here must be answered before any of them is used."""
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255
    p = lambda on: a if on else None   # noqa: E731
    return L.nlsh_probe_ranked_budget(p(z), H if z_stride is None else z_stride, p(code), n, H, key_mode, P, n if n_multi is None else n_multi,
                                      p(uniq), p(offsets), n_buckets, budget, p(keys), p(nkeys), None, None, None)


def test_header_declares_the_call_and_the_abi_is_still_4(L):
    from nlsh_amd import _capi
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    assert re.search(r"\bnlsh_probe_ranked_budget\s*\(", header) and "nlsh_probe_ranked_budget" in _capi.SYMBOLS
    assert hasattr(L, "nlsh_probe_ranked_budget") and len(L.nlsh_probe_ranked_budget.argtypes) == 17
    makefile = open(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "csrc", "Makefile")).read()
    assert "probe_ranked.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, re.M).group(1)
    assert int(re.search(r"#define NLSH_ABI_VERSION (\d+)", header).group(1)) == 4 and L.nlsh_abi_version() == 4


def test_bad_budget_arguments_are_refused_on_the_host(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731
    for budget in (0, -1, -(2 ** 31)):
        assert _call(L, budget=budget) == _capi.E_INVALID and f"budget={budget}" in err()
    for nb in (-1, -70000):
        assert _call(L, n_buckets=nb) == _capi.E_INVALID and f"n_buckets={nb}" in err()
    for missing in ("uniq", "offsets"):
        assert _call(L, **{missing: False}) == _capi.E_INVALID, missing
        assert "null pointer" in err() and "n_buckets=5" in err()


def test_the_refusals_of_the_unbudgeted_call_apply_unchanged(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731
    for missing in ("z", "code", "keys", "nkeys"):
        assert _call(L, **{missing: False}) == _capi.E_INVALID, missing
        assert "null pointer" in err()
    assert _call(L, n=-1) == _capi.E_INVALID and "n=-1" in err()
    assert _call(L, H=16, z_stride=15) == _capi.E_INVALID and "z_stride=15" in err() and "H=16" in err()
    for key_mode in (-1, 2, 7):
        assert _call(L, key_mode=key_mode) == _capi.E_INVALID and f"key_mode={key_mode}" in err()
    for H in (0, 33, -4):
        assert _call(L, H=H, z_stride=64) == _capi.E_UNSUPPORTED
        assert "NLSH_MAX_HASH_BITS" in err() and f"H={H}" in err()
    for P in (0, 129, -1):
        assert _call(L, P=P) == _capi.E_UNSUPPORTED
        assert "NLSH_MAX_ENCODE_PROBES" in err() and f"n_probes={P}" in err()


def test_an_empty_batch_is_ok_without_a_launch(L):
    from nlsh_amd import _capi
    assert _call(L, n=0) == _capi.OK
    assert _call(L, n=0, z=False, code=False, keys=False, nkeys=False, uniq=False, offsets=False, n_buckets=0) == _capi.OK
    assert _call(L, n=0, uniq=False) == _capi.E_INVALID                                 # ... but the index arrays are still checked
    assert _call(L, n=0, budget=0) == _capi.E_INVALID
    assert _call(L, n=0, H=40, z_stride=64) == _capi.E_UNSUPPORTED


# ---------------------------------------------------------------------------- the Python surface
def test_the_budget_keyword_is_checked_before_anything_runs(monkeypatch):
    from nlsh_amd import _capi, hashings
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.indexer import Indexer
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)      # no GPU here; the checks are host logic
    h = hashings.MultivariateBernoulli(MultiLayerRelu(8, [16]), 4, None)
    ix = Indexer.__new__(Indexer)
    ix._hashing, ix.compat, ix.metric = h, False, "l2"
    x = torch.zeros(3, 8)
    calls = {"query": lambda **kw: ix.query(x, **kw), "query_tensors": lambda **kw: ix.query_tensors(x, **kw),
             "hash": lambda **kw: ix.hash(x, hash_times=4, **kw), "hash_device": lambda **kw: ix.hash_device(x, hash_times=4, **kw)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="ranked"):                          # a sampled call has no order to cut
            call(candidate_budget=100, probes="sampled")
        with pytest.raises(ValueError, match="ranked"):                          # ... and neither has a sampled hasher's default
            call(candidate_budget=100)
        for bad in (0, -5):
            with pytest.raises(ValueError, match="candidate_budget"):
                call(candidate_budget=bad, probes="ranked")
        for bad in (2.5, "100", True, [100]):
            with pytest.raises(ValueError, match="candidate_budget"):
                call(candidate_budget=bad, probes="ranked")
        with pytest.raises(ValueError, match="probes"):
            call(candidate_budget=100, probes="nonsense")
        assert h.probes == "sampled", name
        # a valid budget passes the checks and reaches the device requirement: there is no CPU path
        for kw in ({"probes": "ranked"}, {"probes": "ranked", "candidate_budget": np.int64(7)}):
            with pytest.raises(_capi.NlshHipError) as e:
                call(candidate_budget=kw.pop("candidate_budget", 100), **kw)
            assert e.value.code == _capi.E_INVALID and h.probes == "sampled"
    h.probes = "ranked"                                                          # a ranked hasher needs no keyword
    with pytest.raises(_capi.NlshHipError) as e:
        ix.query_tensors(x, candidate_budget=100)
    assert e.value.code == _capi.E_INVALID
    with pytest.raises(ValueError, match="ranked"):                              # ... and the keyword still overrides it
        ix.query_tensors(x, candidate_budget=100, probes="sampled")
    ix.metric = "generic"
    with pytest.raises(NotImplementedError, match="metric"):
        ix.query(x, candidate_budget=100)
    ix.metric = "cosine"
    assert ix._candidate_budget(10 ** 12, "ranked") == rbr.INT32_MAX            # a row holds fewer than 2^31 candidates
