"""CPU-only: host-side validation of the streamed encoder entries (nlsh_encoder_stream_*, nlsh_encode_stream_workspace,
nlsh_encode_hash_stream).  Every call here returns before anything is launched, so no device is needed."""
import os

import pytest

from nlsh_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build_library()
    return _capi.lib()


def _enc(lib, dims, n=1, workspace=None, workspace_bytes=0, packed=16, keys=16, nkeys=16, x=16, x_stride=None, n_probes=1,
         act=_capi.ACT_SIGMOID, key_mode=_capi.KEY_REF_INT16):
    # fake non-null device pointers: validation refuses the call before any of them is read
    return lib.nlsh_encode_hash_stream(x, n, dims[0] if x_stride is None else x_stride, len(dims) - 1, _capi.int_array(dims), packed,
                                       act, key_mode, n_probes, n, 0, 0, None, None, None, keys, nkeys, workspace, workspace_bytes, None)


def test_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    assert "#define NLSH_MAX_STREAM_WIDTH 4096" in header and _capi.MAX_STREAM_WIDTH == 4096
    assert _capi.MAX_WIDTH == 632


def test_wide_encoders_pack_to_a_positive_count(lib):
    dims = [128, 1024, 1024, 16]
    n = lib.nlsh_encoder_stream_packed_floats(3, _capi.int_array(dims))
    assert n == (1024 * 128 + 1024) + (1024 * 1024 + 1024) + (32 * 1024 + 32)
    assert lib.nlsh_encoder_stream_packed_floats(2, _capi.int_array([1024, 4096, 32])) > 0
    assert lib.nlsh_encoder_stream_packed_floats(2, _capi.int_array([25, 633, 8])) > 0
    assert lib.nlsh_encoder_stream_packed_floats(2, _capi.int_array([128, 256, 16])) > 0     # narrow encoders take the form too
    assert lib.nlsh_encoder_stream_packed_floats(1, _capi.int_array([128, 16])) > 0          # no hidden layer


@pytest.mark.parametrize("dims, what", [([128, 4097, 16], b"hidden width 4097"), ([1025, 256, 16], b"input width 1025"),
                                        ([128, 1024, 33], b"hash_size 33"), ([64] * 9 + [16], b"n_layers=9")])
def test_out_of_range_shapes_are_refused(lib, dims, what):
    n_layers = len(dims) - 1
    assert lib.nlsh_encoder_stream_packed_floats(n_layers, _capi.int_array(dims)) == -1
    assert what in lib.nlsh_last_error()
    assert lib.nlsh_encode_stream_workspace(128, n_layers, _capi.int_array(dims)) == 0
    rc = lib.nlsh_encoder_stream_pack(n_layers, _capi.int_array(dims), 16, 16, 16, None)
    assert rc in (_capi.E_INVALID, _capi.E_UNSUPPORTED) and what in lib.nlsh_last_error()
    rc = _enc(lib, dims, workspace=16, workspace_bytes=1 << 30)
    assert rc in (_capi.E_INVALID, _capi.E_UNSUPPORTED) and what in lib.nlsh_last_error()
    if n_layers <= _capi.MAX_LAYERS:
        assert rc == _capi.E_UNSUPPORTED


def test_null_pointers_are_invalid(lib):
    dims = [128, 1024, 1024, 16]
    assert lib.nlsh_encoder_stream_pack(3, _capi.int_array(dims), None, 16, 16, None) == _capi.E_INVALID
    assert lib.nlsh_encoder_stream_pack(3, _capi.int_array(dims), 16, 16, None, None) == _capi.E_INVALID
    assert lib.nlsh_encoder_stream_pack(3, None, 16, 16, 16, None) == _capi.E_INVALID
    assert lib.nlsh_encoder_stream_packed_floats(3, None) == -1
    ws = lib.nlsh_encode_stream_workspace(128, 3, _capi.int_array(dims))
    for kw in (dict(x=None), dict(packed=None), dict(keys=None), dict(nkeys=None), dict(workspace=None)):
        args = dict(workspace=1024, workspace_bytes=ws)
        args.update(kw)
        assert _enc(lib, dims, n=5, **args) == _capi.E_INVALID
        assert b"null pointer" in lib.nlsh_last_error()
    assert _enc(lib, dims, n=0, x=None, packed=None, keys=None, nkeys=None) == _capi.OK     # nothing to do, nothing read


def test_other_arguments_are_checked(lib):
    dims = [128, 1024, 1024, 16]
    ws = lib.nlsh_encode_stream_workspace(128, 3, _capi.int_array(dims))
    assert _enc(lib, dims, workspace=1024, workspace_bytes=ws, x_stride=100) == _capi.E_INVALID
    assert _enc(lib, dims, workspace=1024, workspace_bytes=ws, n_probes=0) == _capi.E_INVALID
    assert _enc(lib, dims, workspace=1024, workspace_bytes=ws, n_probes=_capi.MAX_ENCODE_PROBES + 1) == _capi.E_INVALID
    assert _enc(lib, dims, workspace=1024, workspace_bytes=ws, act=7) == _capi.E_INVALID
    assert _enc(lib, dims, workspace=1024, workspace_bytes=ws, key_mode=7) == _capi.E_INVALID
    assert _enc(lib, dims, n=-1, workspace=1024, workspace_bytes=ws) == _capi.E_INVALID
    assert _enc(lib, dims, workspace=1028, workspace_bytes=ws) == _capi.E_INVALID                    # not 16-byte aligned
    assert b"aligned" in lib.nlsh_last_error()
    assert _enc(lib, dims, workspace=1024, workspace_bytes=ws - 1) == _capi.E_WORKSPACE              # less than one row tile
    assert b"workspace" in lib.nlsh_last_error()


def test_workspace_grows_with_the_rows_per_pass(lib):
    dims = _capi.int_array([128, 1024, 1024, 16])
    sizes = [lib.nlsh_encode_stream_workspace(r, 3, dims) for r in (1, 128, 129, 256, 4096, 1 << 20)]
    assert sizes[0] == sizes[1] > 0                       # one 128-row tile at least
    assert sizes[1] < sizes[2] == sizes[3] < sizes[4] < sizes[5]
    per_row = (2 * 1024 + 32) * 4                         # two activation images + z
    assert sizes[1] == 128 * per_row and sizes[5] == (1 << 20) * per_row
    # one hidden layer: one image
    assert lib.nlsh_encode_stream_workspace(128, 2, _capi.int_array([128, 2048, 16])) == 128 * (2048 + 32) * 4


def test_the_lds_resident_entries_keep_their_limit(lib):
    assert lib.nlsh_encoder_packed_floats(2, _capi.int_array([128, 700, 16])) == -1
    assert lib.nlsh_encoder_packed_floats(2, _capi.int_array([128, 632, 16])) > 0
    assert lib.nlsh_abi_version() == 4


def test_streamed_hashing_is_recognised_and_refuses_the_fused_calls():
    """Host logic of the facade that needs no device: which encoders are streamed, and that they have no fused encode launch."""
    import torch
    from nlsh_amd import hashings
    from nlsh_amd.encoders import MultiLayerRelu

    def hashing(hidden):
        h = hashings.MultivariateBernoulli.__new__(hashings.MultivariateBernoulli)
        h._encoder = MultiLayerRelu(128, hidden)
        h._hash_size = 16
        h._hasher = hashings._Hasher(h._encoder, 16)
        return h
    assert hashing([1024, 1024]).streamed() and hashing([256, 633]).streamed()
    assert not hashing([632, 256]).streamed() and not hashing([256, 256]).streamed()
    with pytest.raises(_capi.NlshHipError) as e:
        hashing([1024, 1024]).encode_args(10, torch.empty((1, 10), dtype=torch.int32), torch.empty((1,), dtype=torch.int32))
    assert e.value.code == _capi.E_UNSUPPORTED and "1024" in str(e.value)
