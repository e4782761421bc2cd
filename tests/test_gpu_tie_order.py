"""The (distance, global row id) order of every top-k path on mass ties: the three scan schedules, their per-query merges, the shard
merge and the reference-typed calls on corpora that hold nothing but copies of a dozen prototypes (tests/tie_ref.py).  Every id list is
compared with `array_equal` against the fp64 reference -- no tie helper: which member of a tie group is returned IS what is tested.
The preconditions (separated prototypes for every query, the kinds of cut and the merge forms reached) are asserted on the CPU by
tests/test_tie_order_cpu.py, which also ties the reference to the oracle."""
import functools

import numpy as np
import pytest
import torch

import tie_ref as T
from helpers import dev, make_hashing
from nlsh_amd import synth
from oracle import oracle

pytestmark = pytest.mark.gpu
METRICS = ["l2", "cosine"]


def _hashing(d, H=4):
    Ws, bs = synth.make_weights([d, 16, H], seed=3)
    return make_hashing(d, (16,), H, Ws, bs, compat=False)


def _distance(metric):
    from nlsh_amd.data import Glove, SIFT
    return SIFT.distance if metric == "l2" else Glove.distance


def _indexer(data, **kw):
    from nlsh_amd.indexer import Indexer
    kw.setdefault("corpus_keys", dev(data.corpus_keys))
    return Indexer(_hashing(data.d), dev(data.corpus), _distance(data.metric), compat=False, **kw)


def _key_table(key_lists):
    """Device key table of caller-supplied lists (a repeated key probes its bucket once, as in Indexer.query_with_keys)."""
    key_lists = [list(dict.fromkeys(int(v) for v in ks)) for ks in key_lists]
    P = max(len(ks) for ks in key_lists)
    tab, cnt = np.zeros((len(key_lists), P), np.int32), np.zeros(len(key_lists), np.int32)
    for i, ks in enumerate(key_lists):
        cnt[i] = len(ks)
        tab[i, :len(ks)] = ks
    return dev(tab), dev(cnt)


@functools.lru_cache(maxsize=None)
def _rows(metric, name, k):
    data = T.dataset(metric, name)
    key_lists = T.key_lists_of(data, k)
    return key_lists, T.candidate_rows(data.corpus_keys, key_lists)


@functools.lru_cache(maxsize=None)
def _oracle(metric, name, k):
    data = T.dataset(metric, name)
    key_lists, _ = _rows(metric, name, k)
    perm, uniq, offs = oracle.build_csr(data.corpus_keys.astype(np.int64))
    qk, nk = oracle.keys_from_lists([list(dict.fromkeys(ks)) for ks in key_lists])
    return oracle.query_batch(data.corpus, perm, uniq, offs, data.queries, qk, nk, k, metric)


def _check(data, rows, k, nc, dist, idx, ids=None, oracle_bits=None):
    """One result against the reference.  ids: global id of every corpus row (default: its number).  oracle_bits: the oracle's
    distances, where the schedule promises them bit for bit (tiled L2)."""
    ids = np.arange(data.N, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    want, d64, ncand = T.expected_topk(data.queries, data.prototypes, data.group_of_row, ids, rows, k, data.metric)
    nc, dist, idx = np.asarray(nc), dist.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(nc, ncand)                                                 # candidate counts: exact
    assert np.array_equal(idx, want)                                                 # the (distance, id) order itself
    ok = want >= 0
    assert np.all(np.isposinf(dist[~ok]))                                            # padding: -1 (above) / +inf
    assert np.all(np.abs(dist[ok].astype(np.float64) - d64[ok]) <= T.DIST_RTOL * np.maximum(1.0, np.abs(d64[ok])))
    order = np.argsort(ids)
    group_of_id = data.group_of_row[order][np.searchsorted(ids[order], np.maximum(want, ids.min()))]
    groups = np.where(ok, group_of_id, -1)
    bits = dist.view(np.uint32)
    for q in range(len(want)):                                                       # one tie group in one row: one bit pattern
        for g in np.unique(groups[q][ok[q]]):
            assert len(np.unique(bits[q][groups[q] == g])) == 1, (q, g)
    if oracle_bits is not None:
        assert np.array_equal(bits, oracle_bits.view(np.uint32))


def _scan_and_check(metric, name, k, ids=None, bits=True, **kw):
    data = T.dataset(metric, name)
    key_lists, rows = _rows(metric, name, k)
    ix = _indexer(data, **kw)
    _, nc, dist, idx = ix.query_with_keys(dev(data.queries), key_lists, k=k)
    tiled_l2 = bits and metric == "l2" and kw.get("algo") == "tiled"
    _check(data, rows, k, nc, dist, idx, ids=ids, oracle_bits=_oracle(metric, name, k)[0] if tiled_l2 else None)
    return ix


# ----------------------------------------------------------------------------- schedules and k
@pytest.mark.parametrize("k", T.NARROW_K)
@pytest.mark.parametrize("algo", ["query", "bucket", "tiled"])
@pytest.mark.parametrize("metric", METRICS)
def test_schedules_on_mass_ties(metric, algo, k):
    _scan_and_check(metric, "main", k, algo=algo)


@pytest.mark.parametrize("k", T.WIDE_K)
@pytest.mark.parametrize("metric", METRICS)
def test_tiled_wide_k_on_mass_ties(metric, k):
    _scan_and_check(metric, "main", k, algo="tiled")


@pytest.mark.parametrize("k", T.NARROW_K)
@pytest.mark.parametrize("algo", ["query", "bucket"])
@pytest.mark.parametrize("metric", METRICS)
def test_segments_of_64_rows_and_their_merges(metric, algo, k):
    """seg_rows = 64: merge_segments_kernel over up to 204 partial lists per query; merge_query with one key per lane, two, one general
    round, several rounds, more than 128 lists and a probe of 33 segments (test_tie_order_cpu.py holds the key lists to these)."""
    _scan_and_check(metric, "lists", k, algo=algo, seg_rows=64)


@pytest.mark.parametrize("k", [10, 129])
@pytest.mark.parametrize("window", [0, 64, 256])
@pytest.mark.parametrize("metric", METRICS)
def test_tiled_shared_windows_on_mass_ties(metric, window, k):
    """A tie group spread over the 1..20-row buckets of one shared window, queries that own different buckets of it."""
    ix = _scan_and_check(metric, "main", k, algo="tiled", window_rows=window)
    assert ix.last_window == window


# ----------------------------------------------------------------------------- ids unrelated to the position
@pytest.mark.parametrize("algo,k", [("query", 33), ("bucket", 10), ("tiled", 64), ("tiled", 129)])
@pytest.mark.parametrize("metric", METRICS)
def test_row_ids_permuted(metric, algo, k):
    """row_ids = a permutation of the global ids: the smallest id of a tie group is not its first row, lane or list."""
    data = T.dataset(metric, "main")
    ids = np.random.default_rng(17).permutation(data.N).astype(np.int32)
    _scan_and_check(metric, "main", k, ids=ids, bits=False, algo=algo, row_ids=dev(ids))


@pytest.mark.parametrize("algo,k", [("bucket", 32), ("tiled", 193)])
def test_id_base_near_the_top_of_the_id_range(algo, k):
    data = T.dataset("l2", "main")
    base = 2 ** 31 - 1 - data.N
    ids = base + np.arange(data.N, dtype=np.int64)
    assert ids[-1] == 2 ** 31 - 2
    _scan_and_check("l2", "main", k, ids=ids, bits=False, algo=algo, id_base=int(base))


# ----------------------------------------------------------------------------- every distance ties
@pytest.mark.parametrize("algo", ["query", "bucket", "tiled"])
@pytest.mark.parametrize("metric", METRICS)
def test_all_identical_corpus(metric, algo):
    """One prototype, ~3000 rows: the result is the k smallest ids of the probed buckets."""
    data = T.dataset(metric, "one")
    for k in (1, 10, 64) + ((129, 256) if algo == "tiled" else ()):
        _scan_and_check(metric, "one", k, algo=algo)
        key_lists, rows = _rows(metric, "one", k)
        want, _, _ = T.expected_topk(data.queries, data.prototypes, data.group_of_row, np.arange(data.N), rows, k, metric)
        for q in (1, 3):
            assert want[q].tolist() == np.sort(rows[q])[:k].tolist()


# ----------------------------------------------------------------------------- row shards + the shard merge
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("metric", METRICS)
def test_row_shards_merged_against_the_whole_corpus_reference(metric, k):
    from nlsh_amd.distributed import merge_topk_device, shard_range
    from nlsh_amd.indexer import Indexer
    data = T.dataset(metric, "main")
    key_lists, rows = _rows(metric, "main", T.WIDE_K[1] if k == 100 else k)          # k = 100 rides on the key lists of k = 128
    keys, nkeys = _key_table(key_lists)
    qd, cd, ck = dev(data.queries), dev(data.corpus), dev(data.corpus_keys)
    keys_all, nc_all = [], []
    for r in range(3):
        lo, hi = shard_range(data.N, r, 3)
        sh = Indexer(_hashing(data.d), cd[lo:hi], _distance(metric), compat=False, corpus_keys=ck[lo:hi].contiguous(), id_base=lo)
        _, _, nc, k64 = sh.scan_tensors(qd, keys, nkeys, k=k, want_keys=True)
        keys_all.append(k64.clone()); nc_all.append(nc.clone())
    packed = torch.cat([torch.stack(keys_all), torch.stack(nc_all).long()[:, :, None]], dim=2)
    dm, im, nm = merge_topk_device(packed, k)
    _check(data, rows, k, nm.cpu().numpy(), dm, im)


# ----------------------------------------------------------------------------- reference-typed paths on a real hasher
def _hashed_index(metric):
    """Keys from a real 4-bit hasher: duplicates hash alike, so a bucket holds thousands of tied rows over many tasks."""
    data = T.dataset(metric, "main")
    ix = _indexer(data, corpus_keys=None)
    assert ix.n_buckets <= 16 and int(ix.bucket_sizes.max()) > 1024
    return data, ix


def _hashed_rows(ix, qd, P, seed):
    """The candidate sets: from the index's own corpus keys and the keys hash_device returns for the seed -- the reference's input."""
    keys, nkeys = ix.hash_device(qd, hash_times=P, seed=seed)
    keys, nkeys = keys.cpu().numpy(), nkeys.cpu().numpy()
    return T.candidate_rows(ix.corpus_keys.cpu().numpy(), [keys[q, :nkeys[q]].tolist() for q in range(len(nkeys))])


@pytest.mark.parametrize("k", [10, 64])
@pytest.mark.parametrize("metric", METRICS)
def test_query_lists_on_mass_ties(metric, k):
    """Indexer.query(): the host-writing merge (merge_finish_ids)."""
    data, ix = _hashed_index(metric)
    qd = dev(data.queries)
    rows = _hashed_rows(ix, qd, 3, seed=21)
    ids, ncand = ix.query(qd, k=k, hash_times=3, seed=21)
    assert ix.last_query_path == "fused"
    want, _, nc = T.expected_topk(data.queries, data.prototypes, data.group_of_row, np.arange(data.N), rows, k, metric)
    assert ncand == nc.tolist() and max(ncand) > 1024
    assert ids == [row[row >= 0].tolist() for row in want]


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("metric", METRICS)
def test_query_tensors_on_mass_ties(metric, k):
    """Indexer.query_tensors(): the fused batch call."""
    data, ix = _hashed_index(metric)
    qd = dev(data.queries)
    rows = _hashed_rows(ix, qd, 3, seed=22)
    dist, idx, nc, _ = ix.query_tensors(qd, k=k, hash_times=3, seed=22)
    _check(data, rows, k, nc.cpu().numpy(), dist, idx)
