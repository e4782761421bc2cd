"""The exact re-rank without a device: the export, every host-side refusal of `nlsh_rerank_topk` through the C ABI with
made-up pointers (a refused call never reads them; tests/test_row_call_checks_cpu.py does this for the row calls), the facade's
refusals, which are raised before any device call, and the numpy statement of the definition (tests/refine_ref.py) against a
brute-force sort."""
import ctypes

import numpy as np
import pytest

from nlsh_amd import _capi
from refine_ref import mono_u32, rerank_reference

OK, INVALID, UNSUPPORTED = _capi.OK, _capi.E_INVALID, _capi.E_UNSUPPORTED
L2, COS, FOLDED = _capi.METRIC_L2_EPS, _capi.METRIC_COSINE, _capi.METRIC_L2_EPS_FOLDED
FAKE = 0x10000          # a 256-byte aligned non-null address: refused calls never dereference it

PARAMS = ("queries", "q_stride", "Q", "d", "store", "store_stride", "n_rows", "id_base", "store_on_host", "store_inv_norm", "cand", "cand_stride",
          "kc", "k", "metric", "out_dist", "out_idx", "out_keys", "out_count", "first_bad", "stream")
VALID = dict(queries=FAKE, q_stride=100, Q=7, d=100, store=FAKE, store_stride=112, n_rows=1000, id_base=0, store_on_host=0, store_inv_norm=FAKE,
             cand=FAKE, cand_stride=40, kc=40, k=10, metric=L2, out_dist=FAKE, out_idx=FAKE, out_keys=FAKE, out_count=FAKE, first_bad=FAKE, stream=None)

FAULTS = [
    ("k = 0", dict(k=0), "k=0", UNSUPPORTED),
    ("k > kc", dict(k=41), "k=41", UNSUPPORTED),
    ("kc > NLSH_MAX_K_TILED", dict(kc=257, cand_stride=257), "kc=257", UNSUPPORTED),
    ("d = 0", dict(d=0), "d=0", UNSUPPORTED),
    ("d > NLSH_MAX_DIM", dict(d=1025, store_stride=1028, q_stride=1025), "d=1025", UNSUPPORTED),
    ("store_stride < d", dict(store_stride=96), "store_stride=96", INVALID),
    ("store_stride not a multiple of 4", dict(store_stride=102), "store_stride=102", INVALID),
    ("store not 16-byte aligned", dict(store=FAKE + 4), "16-byte", INVALID),
    ("cand_stride < kc", dict(cand_stride=39), "cand_stride=39", INVALID),
    ("the folded form", dict(metric=FOLDED), "exact", INVALID),
    ("an unknown metric", dict(metric=9), "metric=9", INVALID),
    ("cosine without norms", dict(metric=COS, store_inv_norm=None), "store_inv_norm", INVALID),
    ("n_rows negative", dict(n_rows=-1), "n_rows=-1", INVALID),
    ("Q negative", dict(Q=-1), "Q=-1", INVALID),
    ("q_stride < d", dict(q_stride=99), "q_stride=99", INVALID),
    ("store_on_host neither 0 nor 1", dict(store_on_host=2), "store_on_host=2", INVALID),
    ("queries null", dict(queries=None), "queries", INVALID),
    ("store null", dict(store=None), "store", INVALID),
    ("cand null", dict(cand=None), "cand", INVALID),
    ("out_dist null", dict(out_dist=None), "out_dist", INVALID),
    ("out_idx null", dict(out_idx=None), "out_idx", INVALID),
    ("first_bad null", dict(first_bad=None), "first_bad", INVALID),
    ("out_keys misaligned", dict(out_keys=FAKE + 4), "out_keys", INVALID),
    # memory the runtime has no record of is not host memory mapped for the device: refused on the host, never read
    ("a host store the runtime does not know", dict(store_on_host=1), "store_on_host", INVALID),
]


def _call(**changes):
    args = dict(VALID, **changes)
    return _capi.lib().nlsh_rerank_topk(*[args[p] for p in PARAMS])


def test_the_library_exports_the_rerank_entry():
    L = ctypes.CDLL(_capi.LIB_PATH)
    assert hasattr(L, "nlsh_rerank_topk")
    assert "nlsh_rerank_topk" in _capi.SYMBOLS
    assert len(_capi.lib().nlsh_rerank_topk.argtypes) == len(PARAMS)
    assert _capi.lib().nlsh_abi_version() == 4      # new entry points only: the ABI version stays


@pytest.mark.parametrize("name,changes,fragment,code", FAULTS, ids=[f[0] for f in FAULTS])
def test_every_refusal_comes_from_the_host_and_names_its_argument(name, changes, fragment, code):
    assert _call(**changes) == code, name
    msg = _capi.lib().nlsh_last_error().decode()
    assert msg.startswith("rerank_topk:") and fragment in msg, msg


def test_an_empty_batch_is_ok_without_a_launch():
    # no pointer of the batch is looked at: the made-up ones would fault if anything were enqueued on them
    assert _call(Q=0) == OK
    assert _call(Q=0, queries=None, cand=None, out_dist=None, out_idx=None, store=None, n_rows=0) == OK
    # ... but the limits are held even for no queries
    assert _call(Q=0, k=0) == UNSUPPORTED
    assert _call(Q=0, metric=FOLDED) == INVALID


def test_out_keys_and_out_count_are_optional():
    # Q = 0 reaches the end of the scalar checks with both null
    assert _call(Q=0, out_keys=None, out_count=None) == OK


# ------------------------------------------------------------------------------------------------ facade refusals, before any device call
class _NoDeviceRows:
    """Stands where the corpus tensor goes: any use of it is a failure of the test (the refusal must come first)."""

    def __getattr__(self, name):
        raise AssertionError(f"the corpus was touched ({name}) before the refusal")


def _bare_indexer(refine="device", refine_factor=4):
    """An `Indexer` with a refine store's bookkeeping and nothing on a device: what the refusals below look at."""
    from nlsh_amd.indexer import Indexer
    ix = Indexer.__new__(Indexer)
    ix.refine, ix.refine_factor, ix.refine_store = refine, refine_factor, object()
    ix.metric, ix.storage, ix.algo, ix.generation = "l2", "float32", None, 0
    return ix


def test_row_ids_with_refine_is_refused_first():
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.multitable import MultiTableIndexer
    with pytest.raises(ValueError, match="row_ids"):
        Indexer(None, _NoDeviceRows(), SIFT.distance, row_ids=object(), refine="device")
    with pytest.raises(ValueError, match="row_ids"):
        MultiTableIndexer([object()], _NoDeviceRows(), SIFT.distance, row_ids=object(), refine="host")
    with pytest.raises(ValueError, match="refine must be"):
        Indexer(None, _NoDeviceRows(), SIFT.distance, refine="disk")
    with pytest.raises(ValueError, match="refine_factor"):
        Indexer(None, _NoDeviceRows(), SIFT.distance, refine="device", refine_factor=0)


@pytest.mark.parametrize("call", ["range_scan_tensors", "range_tensors", "range_query", "range_query_with_keys"])
def test_range_calls_name_refine(call):
    ix = _bare_indexer()
    args = {"range_scan_tensors": (_NoDeviceRows(), None, None, 1.0), "range_tensors": (_NoDeviceRows(), 1.0),
            "range_query": (_NoDeviceRows(), 1.0), "range_query_with_keys": (_NoDeviceRows(), [[0]], 1.0)}[call]
    with pytest.raises(NotImplementedError, match="refine"):
        getattr(ix, call)(*args)


def test_pipeline_and_sharded_index_name_refine():
    from nlsh_amd.data import SIFT
    from nlsh_amd.distributed import ShardedIndexer
    from nlsh_amd.pipeline import QueryPipeline
    with pytest.raises(NotImplementedError, match="refine"):
        QueryPipeline(_bare_indexer(), _NoDeviceRows())
    with pytest.raises(NotImplementedError, match="refine"):
        ShardedIndexer(None, _NoDeviceRows(), SIFT.distance, id_base=0, refine="device")


@pytest.mark.parametrize("call", ["query_tensors", "query", "scan_tensors", "query_with_keys"])
def test_refine_k_out_of_range_is_refused_before_anything_runs(call):
    ix = _bare_indexer()
    lead = {"query_tensors": (_NoDeviceRows(),), "query": (_NoDeviceRows(),), "scan_tensors": (_NoDeviceRows(), None, None),
            "query_with_keys": (_NoDeviceRows(), [[0]])}[call]
    with pytest.raises(ValueError, match="refine_k=5 is less than k=10"):
        getattr(ix, call)(*lead, k=10, refine_k=5)
    with pytest.raises(ValueError, match="refine_k=257"):
        getattr(ix, call)(*lead, k=10, refine_k=257)
    plain = _bare_indexer(refine=None)
    plain.refine_store = None
    with pytest.raises(ValueError, match="refine_k= needs an index built with refine"):
        getattr(plain, call)(*lead, k=10, refine_k=40)


def test_stage_one_k_is_the_stated_convention():
    from nlsh_amd.refine import stage_one_k
    assert [stage_one_k(k, 4) for k in (1, 10, 64, 65, 256)] == [4, 40, 256, 256, 256]
    assert stage_one_k(10, 1) == 10 and stage_one_k(10, 10) == 100 and stage_one_k(100, 10) == 256
    assert stage_one_k(10, 4, refine_k=0) == 0 and stage_one_k(10, 4, refine_k=10) == 10 and stage_one_k(10, 4, refine_k=256) == 256


# ------------------------------------------------------------------------------------------------ the numpy definition against brute force
def test_rerank_reference_against_a_brute_force_sort_with_ties():
    rng = np.random.default_rng(5)
    Q, N, kc, id_base = 6, 50, 30, -20
    # few distinct values, both zeros, negatives, infinities and a NaN: mass ties, ordered by id
    pool = np.array([0.0, -0.0, 1.5, 1.5, -2.0, np.inf, -np.inf, np.nan, 3.25], dtype=np.float32)
    bits = pool[rng.integers(0, len(pool), size=(Q, N))]
    cand = np.stack([rng.choice(np.arange(id_base, id_base + N), kc, replace=False) for _ in range(Q)]).astype(np.int64)
    cand[cand == -1] = 7                    # -1 is padding by definition
    cand[1, 5] = -1
    cand[2, :] = -1
    cand[3, 20:] = -1
    cand[4, 3] = id_base + N                # one past the store: dropped and reported
    cand[5, 0] = id_base - 1
    for k in (1, 10, 30):
        dist, idx, keys, count, first_bad = rerank_reference(bits, cand, k, id_base)
        assert first_bad == 4
        for q in range(Q):
            triples = []
            for i in cand[q].tolist():
                if i != -1 and id_base <= i < id_base + N:
                    b = bits[q, i - id_base]
                    triples.append((int(mono_u32(b.view(np.uint32))), i & 0xFFFFFFFF, i, b))
            triples.sort(key=lambda t: (t[0], t[1]))
            triples = triples[:k]
            n = len(triples)
            assert count[q] == n
            assert idx[q, :n].tolist() == [t[2] for t in triples] and (idx[q, n:] == -1).all()
            assert np.array_equal(dist[q, :n].view(np.uint32), np.array([t[3] for t in triples], dtype=np.float32).view(np.uint32))
            assert np.isposinf(dist[q, n:]).all() and (keys[q, n:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
            assert keys[q, :n].tolist() == [(t[0] << 32) | t[1] for t in triples]
            assert list(keys[q, :n]) == sorted(keys[q, :n])
    # the order of the float order: -inf < negatives < -0 < +0 < positives < +inf < NaN
    order = np.array([-np.inf, -2.0, -0.0, 0.0, 1.5, np.inf, np.nan], dtype=np.float32)
    m = mono_u32(order.view(np.uint32)).astype(np.int64)
    assert (np.diff(m) > 0).all()
