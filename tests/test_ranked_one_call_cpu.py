"""`nlsh_query_batch_ranked` / `nlsh_query_batch_ranked_scratch` without a device: the exports and their declarations, the unchanged ABI
version and descriptor, the scratch size's shape, and every refusal the call makes on the host before it touches the GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(**kw):
    from nlsh_amd import _capi
    dims = _capi.int_array(kw.pop("dims_list", [128, 64, 16]))
    buf = (ctypes.c_char * 65536)()
    a = ctypes.addressof(buf)
    base = dict(n_layers=len(dims) - 1, act=0, key_mode=0, n_probes=10, dims=ctypes.cast(dims, ctypes.c_void_p), packed=a, n_multi_rows=0,
                corpus_sorted=a, row_stride=128, gid=a, uniq_keys=a, offsets=a, bucket_order=a, cell_of=None, cell_offsets=None, inv_norm=None,
                d=128, n_buckets=8, n_cells=0, k=10, metric=0, algo=2, seg_rows=0, hold_done=0, Q=64, qkeys=a, nkeys=a, out_dist=a, out_idx=a,
                out_keys=None, out_ncand=a, status=a, workspace=a, workspace_bytes=65536, max_tasks=16, front=None, plan=None, mid=None, tail=None)
    base.update(kw)
    return _capi.StepDesc(**base), a, (dims, buf)


def _call(desc, a, queries="a", lookup_done=0, budget=0, scratch="a", scratch_bytes=65536, host=None, host_words=0, size=None):
    from nlsh_amd import _capi
    L = _capi.lib()
    pick = lambda v: a if v == "a" else v   # noqa: E731
    return L.nlsh_query_batch_ranked(ctypes.byref(desc), ctypes.sizeof(desc) if size is None else size, pick(queries), 128, lookup_done, budget,
                                     pick(scratch), scratch_bytes, pick(host), host_words, None, None, None)


def test_both_symbols_are_exported_and_declared_and_the_abi_is_still_4():
    from nlsh_amd import _capi
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    for name in ("nlsh_query_batch_ranked_scratch", "nlsh_query_batch_ranked"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _capi.SYMBOLS and hasattr(L, name)
    assert len(L.nlsh_query_batch_ranked.argtypes) == 13 and len(L.nlsh_query_batch_ranked_scratch.argtypes) == 2
    assert L.nlsh_query_batch_ranked_scratch.restype is ctypes.c_size_t
    assert int(re.search(r"#define NLSH_ABI_VERSION (\d+)", header).group(1)) == 4 and L.nlsh_abi_version() == 4


def test_the_descriptor_has_the_size_it_had():
    from nlsh_amd import _capi
    L = _capi.lib()
    assert ctypes.sizeof(_capi.StepDesc) == 264            # 4 + 4 int32, 25 pointers / int64 / size_t words: nlsh_step_desc_t of ABI 4
    d_, a, keep = _desc()
    assert _call(d_, a, size=ctypes.sizeof(d_) - 8) == _capi.E_INVALID
    msg = L.nlsh_last_error()
    assert b"descriptor" in msg and b"264" in msg          # "... this library's is 264": the library's struct agrees


def test_scratch_size_is_positive_monotone_and_zero_on_bad_sizes():
    from nlsh_amd import _capi
    f = _capi.lib().nlsh_query_batch_ranked_scratch
    sizes = {(Q, H): f(Q, H) for Q in (0, 1, 15, 16, 17, 257, 4101, 10 ** 4, 10 ** 6) for H in (1, 8, 14, 16, 20, 32)}
    assert all(v > 0 for v in sizes.values())
    for (Q, H), v in sizes.items():
        assert v >= Q * H * 4 + Q * 4                      # z [Q, H] and the hard codes [Q] at the least
        for (Q2, H2), v2 in sizes.items():
            if Q2 >= Q and H2 >= H:
                assert v2 >= v, ((Q, H), (Q2, H2))
    assert f(10 ** 6, 32) > f(1, 1)
    for Q, H in ((-1, 16), (-10 ** 9, 1), (10, 0), (10, -3), (10, 33), (0, 33), (-1, 0)):
        assert f(Q, H) == 0, (Q, H)


REFUSALS = [
    # (descriptor overrides, call overrides, code name, fragment of the message)
    (dict(), dict(queries=None), "E_INVALID", b"null pointer"),
    (dict(Q=-1), dict(), "E_INVALID", b"Q=-1"),
    (dict(algo=0), dict(), "E_INVALID", b"algo=0"),
    (dict(algo=3), dict(), "E_INVALID", b"algo=3"),
    (dict(n_buckets=0), dict(), "E_INVALID", b"n_buckets=0"),
    (dict(n_probes=0), dict(), "E_UNSUPPORTED", b"n_probes=0"),
    (dict(n_probes=65), dict(), "E_UNSUPPORTED", b"n_probes=65"),
    (dict(n_layers=0), dict(), "E_INVALID", b"n_layers=0"),
    (dict(n_layers=9), dict(), "E_INVALID", b"n_layers=9"),
    (dict(d=100, row_stride=100), dict(), "E_INVALID", b"corpus dimension 100"),      # encoder input 128 vs corpus dimension 100
    (dict(dims_list=[128, 64, 33]), dict(), "E_UNSUPPORTED", b"H=33"),
    (dict(), dict(budget=-1), "E_INVALID", b"budget=-1"),
    (dict(), dict(scratch=None), "E_INVALID", b"scratch is null"),
    (dict(), dict(scratch_bytes=64 * 16 * 4), "E_WORKSPACE", b"scratch of 4096 bytes"),
    (dict(), dict(host="a", host_words=64 * 22 + 1), "E_INVALID", b"words"),           # need 64 * (10 + 1 + 10 + 1) + 2
    (dict(k=65), dict(host="a", host_words=1 << 20), "E_INVALID", b"k=65"),
    (dict(), dict(host="a", host_words=1 << 20), "E_INVALID", b"not host memory mapped"),   # plain process memory, not pinned
    (dict(k=65, algo=1), dict(), "E_UNSUPPORTED", b"k=65"),                             # the scan call's own limits: wave-level schedule, k <= 64
    (dict(workspace_bytes=256), dict(), "E_WORKSPACE", b"workspace"),
]


@pytest.mark.parametrize("dkw,ckw,code,fragment", REFUSALS, ids=[f"{i}-{r[3].decode().replace(' ', '_')}" for i, r in enumerate(REFUSALS)])
def test_every_refusal_is_a_code_and_a_message(dkw, ckw, code, fragment):
    from nlsh_amd import _capi
    L = _capi.lib()
    d_, a, keep = _desc(**dkw)
    assert _call(d_, a, **ckw) == getattr(_capi, code), L.nlsh_last_error()
    assert fragment in L.nlsh_last_error(), L.nlsh_last_error()


def test_a_null_descriptor_is_refused_and_an_empty_batch_is_ok():
    from nlsh_amd import _capi
    L = _capi.lib()
    d_, a, keep = _desc()
    assert L.nlsh_query_batch_ranked(None, ctypes.sizeof(d_), a, 128, 0, 0, a, 65536, None, 0, None, None, None) == _capi.E_INVALID
    d0, a0, keep0 = _desc(Q=0)
    assert _call(d0, a0, queries=None) == _capi.OK                       # nothing to do: no launch, no pointer is looked at
    assert _call(d0, a0, queries=None, lookup_done=1, budget=5) == _capi.OK
