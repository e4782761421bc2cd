"""Likelihood-ranked probes, the parts that need no device: the two forms of the Python reference against each other (the GPU tests
rely on the heap form), `nlsh_probe_ranked`'s host-side refusals through the C ABI, and the facade's refusal of an unknown mode."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ranked_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {"random": rr.random_rows, "ties": rr.tie_rows, "absorbing": rr.absorbing_rows}


@pytest.fixture(scope="module")
def L():
    from nlsh_amd import _capi
    return _capi.lib()


# ---------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("kind", sorted(ROWS))
@pytest.mark.parametrize("H", range(1, 11))
def test_best_first_equals_the_sorted_enumeration(kind, H):
    z = ROWS[kind](4, H, seed=100 * H + len(kind))
    codes = rr.hard_codes(z, H)
    for key_mode in (rr.KEY_REF_INT16, rr.KEY_FULL):
        for P in (1, 2, 7, 64, 128):
            for r in range(z.shape[0]):
                want = rr.brute(z[r], int(codes[r]), H, P, key_mode)
                got = rr.best_first(z[r], int(codes[r]), H, P, key_mode)
                assert got == want, (kind, H, P, key_mode, r)
                assert len(want[0]) == min(P, 1 << H) and want[0][0] == rr.key_of(int(codes[r]), key_mode) and want[1][0] == 0
                assert want[1] == sorted(want[1])                        # costs ascend (non-negative floats: bit order is value order)


def test_the_tie_and_absorbing_rows_do_tie():
    """The rows are only worth their name if chains really round to equal costs: the mask then decides the order."""
    for kind in ("ties", "absorbing"):
        z = ROWS[kind](4, 10, seed=3)
        assert any(len(set(rr.brute(z[r], 0, 10, 128, rr.KEY_FULL)[1])) < 100 for r in range(4)), kind
    z = rr.absorbing_rows(64, 10, seed=3)
    assert np.isinf(z).any() and (np.abs(z[np.isfinite(z)]).min() <= 1e-6) and (np.abs(z[np.isfinite(z)]).max() >= 1e6)


def test_all_zero_row_enumerates_the_masks_in_order():
    H, P = 6, 64
    keys, costs = rr.best_first(np.array([0.0, -0.0] * 3, dtype=np.float32), 0b101010, H, P, rr.KEY_FULL)
    # every cost is +0: the order is mask 0, 1, 2, ...; sorted position i is bit index i (ties by h), i.e. code bit H-1-i
    want = [0b101010 ^ int(format(m, "06b")[::-1], 2) for m in range(P)]
    assert keys == want and costs == [0] * P


def test_int16_keys_of_wide_codes_collide_and_are_dropped_in_first_occurrence_order():
    H = 20
    z = np.full((H,), 5.0, dtype=np.float32)
    z[:4] = [0.1, 0.2, 0.3, 0.4]                       # the four cheapest flips sit in code bits 19..16: invisible to a 16-bit key
    keys, costs = rr.best_first(z, 0xABCDE, H, 16, rr.KEY_REF_INT16)
    assert keys == [rr.key_of(0xABCDE, rr.KEY_REF_INT16)] and costs == [0]
    full, _ = rr.best_first(z, 0xABCDE, H, 16, rr.KEY_FULL)
    assert len(set(full)) == 16


# ---------------------------------------------------------------------------- the C ABI's host-side checks
def _call(L, z=True, code=True, keys=True, nkeys=True, n=8, H=16, z_stride=None, key_mode=1, P=10, n_multi=None):
    """nlsh_probe_ranked with pointers into a small host buffer: every call here must be answered before any of them is used."""
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255
    p = lambda on: a if on else None   # noqa: E731
    return L.nlsh_probe_ranked(p(z), H if z_stride is None else z_stride, p(code), n, H, key_mode, P, n if n_multi is None else n_multi,
                               p(keys), p(nkeys), None, None)


def test_header_declares_the_call_and_the_abi_is_still_4(L):
    from nlsh_amd import _capi
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    assert re.search(r"\bnlsh_probe_ranked\s*\(", header) and "nlsh_probe_ranked" in _capi.SYMBOLS
    makefile = open(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "csrc", "Makefile")).read()
    assert "probe_ranked.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, re.M).group(1)
    assert int(re.search(r"#define NLSH_ABI_VERSION (\d+)", header).group(1)) == 4 and L.nlsh_abi_version() == 4


def test_bad_arguments_are_refused_on_the_host(L):
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
    assert _call(L, n=0, z=False, code=False, keys=False, nkeys=False) == _capi.OK      # an empty tensor's pointer is NULL
    assert _call(L, n=0, H=40, z_stride=64) == _capi.E_UNSUPPORTED                      # ... but the shape is still checked


# ---------------------------------------------------------------------------- the Python surface
def test_an_unknown_probe_mode_is_a_value_error_everywhere(monkeypatch):
    from nlsh_amd import _capi, hashings
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.indexer import Indexer
    assert _capi.PROBES == ("sampled", "ranked")
    with pytest.raises(ValueError, match="probes"):
        hashings.MultivariateBernoulli(MultiLayerRelu(8, [16]), 4, None, probes="nonsense")
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)      # no GPU here; the mode is host logic
    h = hashings.MultivariateBernoulli(MultiLayerRelu(8, [16]), 4, None)
    assert h.probes == "sampled" and hashings.MultivariateBernoulli.probes == "sampled"
    assert hashings.MultivariateBernoulli(MultiLayerRelu(8, [16]), 4, None, probes="ranked").probes == "ranked"
    x = torch.zeros(3, 8)
    for call in (lambda: h.hash(x, n=2, probes="nonsense"), lambda: h.hash_device(x, n=2, probes="nonsense")):
        with pytest.raises(ValueError, match="probes"):
            call()
    h.probes = "nonsense"                                                        # a mistyped attribute is found at the next call
    with pytest.raises(ValueError, match="probes"):
        h.hash_device(x, n=2)
    h.probes = "sampled"
    ix = Indexer.__new__(Indexer)
    ix._hashing, ix.compat, ix.metric = h, False, "l2"
    for call in (lambda: ix.query(x, probes="nonsense"), lambda: ix.query_tensors(x, probes="nonsense"),
                 lambda: ix.hash(x, hash_times=2, probes="nonsense"), lambda: ix.hash_device(x, hash_times=2, probes="nonsense")):
        with pytest.raises(ValueError, match="probes"):
            call()
        assert h.probes == "sampled"
    # a valid mode passes the check and reaches the device requirement: there is no CPU path, and the attribute is restored on that exit
    for call in (lambda: ix.query_tensors(x, probes="ranked"), lambda: ix.hash_device(x, hash_times=2, probes="ranked"),
                 lambda: h.hash_device(x, n=2, probes="ranked")):
        with pytest.raises(_capi.NlshHipError) as e:
            call()
        assert e.value.code == _capi.E_INVALID and h.probes == "sampled"


def test_a_ranked_hasher_has_no_fused_encode_call(monkeypatch):
    from nlsh_amd import _capi, hashings
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.indexer import Indexer
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    h = hashings.MultivariateBernoulli(MultiLayerRelu(8, [16]), 4, None, probes="ranked")
    with pytest.raises(_capi.NlshHipError) as e:
        h.encode_args(10, torch.empty((1, 10), dtype=torch.int32), torch.empty((1,), dtype=torch.int32))
    assert e.value.code == _capi.E_UNSUPPORTED and "ranked" in str(e.value)
    ix = Indexer.__new__(Indexer)
    ix._hashing, ix.metric, ix.n_buckets = h, "l2", 7
    q = torch.zeros(100, 8)
    assert ix._fuses(q, 10, _capi.SCAN_BUCKET_TILED) is False
    h.probes = "sampled"
    assert ix._fuses(q, 10, _capi.SCAN_BUCKET_TILED) is True
