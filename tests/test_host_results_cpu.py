"""`nlsh_query_batch_host`: the refusals that are decided on the host before any HIP call -- a missing result block, one that is too
small for `ids | counts | status | key rows`, and k beyond the host-writing merge -- so they are checked without a device."""
import ctypes


def _desc(**kw):
    from nlsh_amd import _capi
    dims = _capi.int_array([128, 64, 16])
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    base = dict(n_layers=2, act=0, key_mode=0, n_probes=10, dims=ctypes.cast(dims, ctypes.c_void_p), packed=a, n_multi_rows=0,
                corpus_sorted=a, row_stride=128, gid=a, uniq_keys=a, offsets=a, bucket_order=a, cell_of=None, cell_offsets=None, inv_norm=None,
                d=128, n_buckets=8, n_cells=0, k=10, metric=0, algo=2, seg_rows=0, hold_done=0, Q=64, qkeys=a, nkeys=a, out_dist=a, out_idx=a,
                out_keys=None, out_ncand=a, status=a, workspace=a, workspace_bytes=4096, max_tasks=16, front=None, plan=None, mid=None, tail=None)
    base.update(kw)
    return _capi.StepDesc(**base), a, (dims, buf)


def test_query_batch_host_refuses_null_small_and_wide_k_on_the_host():
    from nlsh_amd import _capi
    L = _capi.lib()
    d_, a, keep = _desc()
    need = 64 * 10 + 64 + 2 + 64 * 11

    def call(desc, out, words):
        return L.nlsh_query_batch_host(ctypes.byref(desc), ctypes.sizeof(desc), a, 128, 1, 0, 0, out, words, None)

    assert call(d_, None, need) == _capi.E_INVALID
    assert b"host_out is null" in L.nlsh_last_error()
    assert call(d_, a, need - 1) == _capi.E_INVALID
    msg = L.nlsh_last_error()
    assert b"words" in msg and str(need).encode() in msg
    wide, a2, keep2 = _desc(k=65)
    assert call(wide, a2, 1 << 20) == _capi.E_INVALID
    assert b"k=65" in L.nlsh_last_error()
    qm, a3, keep3 = _desc(algo=0)
    assert call(qm, a3, 1 << 20) == _capi.E_INVALID            # the query-major schedule has no host-writing merge
    assert b"algo=0" in L.nlsh_last_error()
    assert L.nlsh_query_batch_host(ctypes.byref(d_), ctypes.sizeof(d_) - 8, a, 128, 1, 0, 0, a, need, None) == _capi.E_INVALID
    assert b"descriptor" in L.nlsh_last_error()
