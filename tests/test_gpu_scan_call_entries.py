"""The equivalence `Indexer._scan_launch` rests on: on a float32 index the plain call (`nlsh_scan_topk_cells_phase`), the typed call with
`NLSH_STORE_F32` and the filtered call with a NULL filter are ONE call -- the raw bits of `out_dist`, `out_idx`, `out_keys` and `out_ncand`
are equal across the three, on every schedule, for both metrics, narrow and wide k, with and without shared windows.  (The facade goes
through the filtered entry for every index, so the tests that compare a direct call against `scan_tensors` no longer hold the entries
against each other; this one does, entry against entry, each into buffers and a workspace of its own.)"""
import numpy as np
import pytest
import torch

from helpers import dev
from nlsh_amd import _capi
from test_gpu_corpus_storage import _dist, _hasher, _same

pytestmark = pytest.mark.gpu

N, D, Q, P = 600, 20, 33, 3
# 40 buckets: one of 300 rows (two 256-row segments), a few mid-sized ones, many under 64 rows -- some of 1..3 rows: shared windows
SIZES = (300, 70, 40, 30) + (12,) * 5 + (5,) * 6 + (3,) * 9 + (1,) * 8 + (2,) * 7 + (0,)
MAX_TASKS = 1024
_world = {}


def world(metric):
    if metric not in _world:
        from nlsh_amd.indexer import Indexer
        sizes = list(SIZES)
        sizes[-1] = N - sum(sizes)
        assert len(sizes) == 40 and sizes[-1] > 0 and max(sizes) > 256 and sum(s < 64 for s in sizes) >= 30
        rng = np.random.default_rng(11)
        bucket_keys = np.sort(rng.choice(np.arange(-500, 500), size=len(sizes), replace=False)).astype(np.int32)
        corpus_keys = rng.permutation(np.repeat(bucket_keys, sizes)).astype(np.int32)
        rows = rng.standard_normal((N, D)).astype(np.float32)
        ix = Indexer(_hasher(D), dev(rows), _dist(metric), corpus_keys=dev(corpus_keys), compat=False)
        # every query probes the big bucket or a small one, a random one, and a key no bucket has (or a repeat): P = 3, some rows with 2 keys
        keys = np.stack([np.where(np.arange(Q) % 2 == 0, bucket_keys[np.argmax(sizes)], bucket_keys[-3]),
                         rng.choice(bucket_keys, size=Q), np.where(np.arange(Q) % 3 == 0, 9999, rng.choice(bucket_keys, size=Q))], axis=1)
        nkeys = np.where(np.arange(Q) % 5 == 4, 2, P)
        q = dev(rows[rng.integers(0, N, size=Q)] + rng.standard_normal((Q, D)).astype(np.float32) * 0.1)
        _world[metric] = ix, q, dev(keys.astype(np.int32)), dev(nkeys.astype(np.int32))
    return _world[metric]


def _call(ix, entry, q, keys, nkeys, k, algo, window):
    """One call of `entry` ("plain" | "typed" | "filtered") into fresh outputs and a fresh zeroed workspace -> (dist, idx, keys64, ncand)."""
    from nlsh_amd.indexer import _SCAN_ARGS_AFTER_QUERIES, _SCAN_ARGS_BEFORE_QUERIES
    L = _capi.lib()
    out_dist, _, out_idx, ncand, status, out_keys = ix._outputs(Q, k, q.device, True)
    ws = torch.zeros((L.nlsh_scan_workspace(Q, P, k, MAX_TASKS, ix.n_buckets, D),), dtype=torch.uint8, device=q.device)
    f = ix._scan_fields(Q, D, keys, nkeys, k, algo, MAX_TASKS, out_dist, out_idx, out_keys, ncand, status, ws, window)
    before, after = _SCAN_ARGS_BEFORE_QUERIES(f), _SCAN_ARGS_AFTER_QUERIES(f)
    tail = (None, None, torch.cuda.current_stream().cuda_stream, _capi.PHASE_ALL)
    if entry == "plain":
        rc = L.nlsh_scan_topk_cells_phase(*before, q.data_ptr(), q.stride(0), *after, *tail)
    elif entry == "typed":
        rc = L.nlsh_scan_topk_cells_phase_typed(before[0], _capi.STORE_F32, *before[1:], q.data_ptr(), q.stride(0), *after, *tail)
    else:
        rc = L.nlsh_scan_topk_cells_phase_filtered(before[0], _capi.STORE_F32, *before[1:], q.data_ptr(), q.stride(0), *after, *tail, None)
    _capi.check(rc)
    assert status.cpu().tolist()[1] == 0          # the task table held the batch
    return out_dist, out_idx, out_keys, ncand


CASES = [(_capi.SCAN_BUCKET_TILED, k, window) for k in (5, 70) for window in (0, 64)] + \
        [(_capi.SCAN_QUERY_MAJOR, 5, 0), (_capi.SCAN_BUCKET_MAJOR, 5, 0)]


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("algo, k, window", CASES)
def test_plain_typed_f32_and_null_filter_calls_are_one_call(metric, algo, k, window):
    ix, q, keys, nkeys = world(metric)
    plain = _call(ix, "plain", q, keys, nkeys, k, algo, window)
    assert int((plain[1] >= 0).sum()) > Q and int(plain[3].max()) > 256        # real lists, and a query with more than one segment of candidates
    for entry in ("typed", "filtered"):
        got = _call(ix, entry, q, keys, nkeys, k, algo, window)
        for a, b, name in zip(got, plain, ("out_dist", "out_idx", "out_keys", "out_ncand")):
            _same(a, b, (entry, name))
