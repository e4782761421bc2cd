"""nlsh_exact_topk / nlsh_exact_workspace, the parts that need no device: the symbols against the header, the workspace size as a function
of its arguments, the host-side argument checks (nothing is launched and no pointer is read before they pass) and the facade's refusal
of host tensors."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from nlsh_amd import _capi
    return _capi.lib()


def _topk(L, N=1000, d=128, Q=10, k=10, metric=0, row_stride=None, q_stride=None, self_row0=-1, splits=1, ws_bytes=None):
    """nlsh_exact_topk with pointers into a small host buffer: every call here must be refused before any of them is used."""
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255
    need = L.nlsh_exact_workspace(Q, N, k, splits) or (1 << 20)
    return L.nlsh_exact_topk(a, d if row_stride is None else row_stride, N, d, a, d if q_stride is None else q_stride, Q, k, metric,
                             self_row0, splits, a, a, a, need if ws_bytes is None else ws_bytes, None)


def test_header_and_library_agree_and_the_abi_is_still_4(L):
    from nlsh_amd import _capi
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    for sym in ("nlsh_exact_workspace", "nlsh_exact_topk"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in _capi.SYMBOLS
        getattr(L, sym)
    assert re.search(r"#define NLSH_EXACT_L2 0\b", header) and re.search(r"#define NLSH_EXACT_COSINE 1\b", header)
    assert (_capi.EXACT_L2, _capi.EXACT_COSINE) == (0, 1)
    assert int(re.search(r"#define NLSH_ABI_VERSION (\d+)", header).group(1)) == 4 and L.nlsh_abi_version() == 4


def test_workspace_is_zero_for_invalid_arguments(L):
    assert L.nlsh_exact_workspace(100, 1000, 10, 0) > 0
    assert L.nlsh_exact_workspace(0, 0, 1, 0) > 0            # Q = 0 and N = 0 are valid
    for Q, N, k, splits in ((100, 1000, 0, 0), (100, 1000, 257, 0), (-1, 1000, 10, 0), (100, 1 << 31, 10, 0), (100, -1, 10, 0),
                            (100, 1000, 10, -1)):
        assert L.nlsh_exact_workspace(Q, N, k, splits) == 0, (Q, N, k, splits)
    assert L.nlsh_exact_workspace(100, (1 << 31) - 1, 10, 0) > 0


def test_workspace_is_monotone(L):
    ws = L.nlsh_exact_workspace
    for splits in (1, 4):
        sizes = [ws(Q, 50000, 100, splits) for Q in (0, 1, 127, 128, 129, 1000, 4096, 65536)]
        assert sizes == sorted(sizes) and sizes[0] > 0, sizes
    sizes = [ws(1000, 50000, k, 2) for k in (1, 10, 64, 65, 100, 128, 200, 256)]
    assert sizes == sorted(sizes), sizes
    sizes = [ws(1000, 50000, 100, s) for s in (1, 2, 3, 7, 8, 64)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0], sizes
    # automatic splits: a function of Q alone inside the workspace, so Q-monotone at fixed N and k is not implied; it is bounded instead
    assert ws(1000, 50000, 100, 0) <= ws(1000, 50000, 100, 64)


@pytest.mark.parametrize("splits", [0, 1, 5])
def test_workspace_depends_on_n_through_the_norm_array_only(L, splits):
    ws = L.nlsh_exact_workspace
    for Q, k in ((1, 1), (300, 100), (65536, 256)):
        base = ws(Q, 0, k, splits)
        for N in (1, 1000, 1037, 10 ** 6, 10 ** 8, (1 << 31) - 1):
            extra = ws(Q, N, k, splits) - base
            assert 4 * N <= extra < 4 * N + 256, (Q, k, N, extra)      # the norms, rounded up to the workspace's 256-byte alignment
    # the rest is O(splits * Q * k): no more than a constant number of keys per (split, query) list
    assert ws(1000, 0, 100, 4) <= 4 * 1000 * 512 * 8 + 4 * 1000 + 4096


def test_bad_arguments_are_refused_on_the_host(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731
    for d in (0, 1025, -3):
        assert _topk(L, d=d, row_stride=2048, q_stride=2048) == _capi.E_UNSUPPORTED
        assert "NLSH_MAX_DIM" in err() and "1024" in err() and f"d={d}" in err()
    for k in (0, 257, -1):
        assert _topk(L, k=k) == _capi.E_UNSUPPORTED
        assert "NLSH_MAX_K_TILED" in err() and "256" in err() and f"k={k}" in err()
    for metric in (2, -1, 7):
        assert _topk(L, metric=metric) == _capi.E_INVALID
        assert "NLSH_EXACT_L2" in err() and "NLSH_EXACT_COSINE" in err()
    assert _topk(L, row_stride=127) == _capi.E_INVALID and "row_stride=127" in err() and "d=128" in err()
    assert _topk(L, q_stride=100) == _capi.E_INVALID and "q_stride=100" in err()
    assert _topk(L, N=1 << 31) == _capi.E_UNSUPPORTED and "2^31" in err()
    assert _topk(L, Q=-1) == _capi.E_INVALID
    assert _topk(L, self_row0=-2) == _capi.E_INVALID and "self_row0" in err()
    assert _topk(L, splits=-1) == _capi.E_INVALID and "splits" in err()


def test_short_workspace_is_refused(L):
    from nlsh_amd import _capi
    need = L.nlsh_exact_workspace(10, 1000, 10, 1)
    for have in (0, 16, need - 1):
        assert _topk(L, ws_bytes=have) == _capi.E_WORKSPACE
        msg = L.nlsh_last_error().decode()
        assert str(need) in msg and str(have) in msg and "nlsh_exact_workspace" in msg
    assert _topk(L, Q=0) == _capi.OK                 # an empty batch passes every check and launches nothing
    assert _topk(L, Q=0, ws_bytes=0) == _capi.OK


def test_facade_refuses_host_tensors():
    from nlsh_amd import _capi, exact
    q, c = torch.zeros(4, 8), torch.zeros(10, 8)
    for args in ((q, c, 2), (q.numpy(), c.numpy(), 2), (None, c, 2)):
        with pytest.raises(_capi.NlshHipError) as e:
            exact.exact_topk(*args)
        assert e.value.code == _capi.E_INVALID and "no CPU path" in str(e.value)
    with pytest.raises(_capi.NlshHipError) as e:
        exact.self_knn(c, 3)
    assert e.value.code == _capi.E_INVALID
