"""MultiTableIndexer against ITS DEFINITION: the result of a query is the top-k by (distance bits, id) of the UNION of the T tables'
candidate sets, every row once.  Three references, none of them the code under test: the numpy unique merge of the tables' own
`query_tensors(want_keys=True)` results (multi_table_ref), a host-built union of candidate sets ranked by fp64 distances on data whose
ties are exact copies, and -- for mutation and filters -- a freshly built index over the rows that should be left.  The first test
guards the premise of all of it: a row reached through two tables carries ONE distance word."""
import numpy as np
import pytest
import torch

import multi_table_ref as M
from helpers import dev, fp64_distances, make_hashing
from nlsh_amd import _capi, synth

pytestmark = pytest.mark.gpu

CENTRE = {None: (0.0, 1.0), "float32": (0.0, 1.0), "float16": (0.0, 4.0), "uint8": (127.5, 74.0)}     # (mean, spread) of the stored values
SEED = 20


def _dist(metric):
    from nlsh_amd.data import Glove, SIFT
    return SIFT.distance if metric == "l2" else Glove.distance


def _hashers(d, H, T, storage=None, mean=None, spread=None):
    """T untrained MLP hashers that differ in their weight seed; the first layer standardises the value range of the rows."""
    m0, s0 = CENTRE[storage]
    mean, spread = (m0 if mean is None else mean), (s0 if spread is None else spread)
    out = []
    for t in range(T):
        Ws, bs = synth.make_weights([d, 32, H], seed=1000 + 17 * t + d)
        Ws[0] = (Ws[0] / spread).astype(np.float32)
        bs[0] = (bs[0] - Ws[0].sum(1) * mean).astype(np.float32)
        out.append(make_hashing(d, (32,), H, Ws, bs, compat=False))
    return out


def _rows(storage, n, d, rng):
    """float32 [n, d] values the storage holds exactly."""
    if storage == "uint8":
        return rng.integers(0, 256, size=(n, d)).astype(np.float32)
    if storage == "float16":
        return (rng.standard_normal((n, d)) * 4).astype(np.float16).astype(np.float32)
    return rng.standard_normal((n, d)).astype(np.float32)


def _queries(storage, Q, d, rng, corpus):
    """Half the queries sit next to corpus rows, half are fresh draws."""
    q = _rows(storage, Q, d, rng)
    near = rng.integers(0, len(corpus), size=Q)
    q[::2] = corpus[near[::2]]
    return (q + rng.standard_normal((Q, d)).astype(np.float32) * np.float32(0.05 * CENTRE[storage][1])).astype(np.float32)


def _multi(hashers, corpus, metric="l2", **kw):
    from nlsh_amd.multitable import MultiTableIndexer
    return MultiTableIndexer(hashers, corpus if isinstance(corpus, torch.Tensor) else dev(corpus), _dist(metric), **kw)


def _np64(t):
    return t.cpu().numpy().view(np.uint64)


def _per_table(mt, q, filters=None, **kw):
    """The tables' own results -> (keys uint64 [T, Q, k], counts int32 [T, Q])."""
    keys, counts = [], []
    for t, table in enumerate(mt.tables):
        _, _, nc, k64 = table.query_tensors(q, want_keys=True, filter=None if filters is None else filters.filters[t], **kw)
        keys.append(_np64(k64))
        counts.append(nc.cpu().numpy())
    return np.stack(keys), np.stack(counts)


def _assert_is_the_merge(got, keys_all, counts_all, k, what):
    dist, idx, ncand, keys = got
    want_dist, want_idx, want_keys = M.unique_merge_reference(keys_all, k)
    assert np.array_equal(_np64(keys), want_keys), what
    assert np.array_equal(idx.cpu().numpy(), want_idx), what
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), want_dist.view(np.uint32)), what
    assert np.array_equal(ncand.cpu().numpy(), counts_all.sum(0, dtype=np.int64).astype(np.int32)), what


def _same(a, b, what):
    """Two result tuples, word for word."""
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        x, y = x.contiguous(), y.contiguous()
        assert x.dtype == y.dtype and x.shape == y.shape, what
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), what


# ---------------------------------------------------------------------------------------------- the premise
@pytest.mark.parametrize("storage", ["float32", "float16", "uint8"])
@pytest.mark.parametrize("form", ["l2", "folded", "cosine"])
def test_a_row_has_one_distance_word_in_every_table(form, storage):
    """Three tables, k = 256, enough probes that the lists overlap: every id seen by more than one table carries ONE 64-bit key."""
    rng = np.random.default_rng([SEED, len(form), len(storage)])
    N, d, Q = 2000, 100, 33
    corpus = _rows(storage, N, d, rng)
    q = dev(_queries(storage, Q, d, rng, corpus))
    metric = "cosine" if form == "cosine" else "l2"
    mt = _multi(_hashers(d, 6, 3, storage), corpus, metric, storage=storage, l2_form="folded" if form == "folded" else "exact")
    assert [t.storage for t in mt.tables] == [storage] * 3 and all(t.algo == "tiled" and not t.compat for t in mt.tables)
    keys_all, _ = _per_table(mt, q, k=256, hash_times=8, probes="ranked")
    shared = 0
    for qi in range(Q):
        flat = keys_all[:, qi].reshape(-1)
        flat = flat[flat != M.KEY_NONE]
        uniq = np.unique(flat)
        assert len(np.unique(uniq & M.LOW32)) == len(uniq), (form, storage, qi)      # an id with two distance words would be two keys
        shared += len(flat) - len(uniq)
    assert shared > Q * 20, shared                                                   # the lists did overlap


# ---------------------------------------------------------------------------------------------- query_tensors = merge of the tables' calls
_SHAPES = [(2000, 8, 5, 2), (2000, 1, 1, 3), (20000, 100, 257, 3), (20000, 128, 5, 1), (2000, 100, 257, 2)]       # N, d, Q, T


@pytest.mark.parametrize("N, d, Q, T", _SHAPES)
def test_query_tensors_is_the_unique_merge_of_the_tables_results(N, d, Q, T):
    rng = np.random.default_rng([SEED, N, d, Q, T])
    corpus = _rows(None, N, d, rng)
    q = dev(_queries(None, Q, d, rng, corpus))
    mt = _multi(_hashers(d, 6 if N == 2000 else 9, T), corpus)
    assert len(mt.tables) == T and mt.n_tables == T
    for k in (1, 10, 100, 256):
        for kw in (dict(probes="sampled", seed=7, hash_times=4), dict(probes="ranked", hash_times=3),
                   dict(probes="ranked", hash_times=12, candidate_budget=150)):
            keys_all, counts_all = _per_table(mt, q, k=k, **kw)
            got = mt.query_tensors(q, k=k, want_keys=True, **kw)
            _assert_is_the_merge(got, keys_all, counts_all, k, (N, d, Q, T, k, kw))
            three = mt.query_tensors(q, k=k, **kw)                                   # without keys: the same first three tensors
            assert len(three) == 3
            _same(three, got[:3], "want_keys=False")
    assert mt.tables[0].last_algo == _capi.SCAN_BUCKET_TILED                         # also at Q = 1: the schedule never depends on Q x P


@pytest.mark.parametrize("storage", ["float16", "uint8"])
@pytest.mark.parametrize("window", [0, 64, None])
def test_storages_and_windows(storage, window):
    rng = np.random.default_rng([SEED, len(storage), 0 if window is None else window + 1])
    N, d, Q = 2000, 100, 37
    corpus = _rows(storage, N, d, rng)
    q = dev(_queries(storage, Q, d, rng, corpus))
    mt = _multi(_hashers(d, 7, 3, storage), corpus, storage=storage, window_rows=window)
    plain = _multi([t._hashing for t in mt.tables], corpus, window_rows=64, corpus_keys=[t.corpus_keys for t in mt.tables])   # float32 twin
    for k in (10, 100):
        kw = dict(k=k, hash_times=5, probes="ranked")
        keys_all, counts_all = _per_table(mt, q, **kw)
        got = mt.query_tensors(q, want_keys=True, **kw)
        _assert_is_the_merge(got, keys_all, counts_all, k, (storage, window, k))
        _same(got, plain.query_tensors(q, want_keys=True, **kw), "a compressed multi-table index is the float32 one over the same values")


# ---------------------------------------------------------------------------------------------- against the definition, end to end
def _separated_world(d, hi, rng, n_proto=40, n_queries=16):
    """Integer-valued prototypes and queries in [0, hi) such that, for every query, two different prototypes never share an integer
    squared distance: every exact tie of the corpus is then a tie between COPIES of one prototype (same vectors, same device bits), and
    fp64 numpy distances order everything else as any fp32 evaluation does.  Even queries are a prototype with one coordinate moved by
    one (they share its bucket in most tables), odd ones are fresh draws; a draw that breaks the rule is drawn again."""
    protos = np.unique(rng.integers(0, hi, size=(n_proto, d)), axis=0).astype(np.float32)
    assert len(protos) == n_proto
    queries = []
    while len(queries) < n_queries:
        if len(queries) % 2:
            qv = rng.integers(0, hi, size=d).astype(np.float32)
        else:
            qv = protos[rng.integers(n_proto)].copy()
            c = rng.integers(d)
            qv[c] += 1.0 if qv[c] < hi - 1 else -1.0
        d2 = ((protos - qv) ** 2).sum(1).astype(np.int64)
        if d2.min() > 0 and len(np.unique(d2)) == n_proto:
            queries.append(qv)
    return protos, np.stack(queries)


@pytest.mark.parametrize("d", [8, 128])
def test_results_are_the_topk_of_the_united_candidate_sets(d):
    rng = np.random.default_rng([SEED, d, 3])
    hi = 16 if d == 8 else 8                                                         # squared distances stay small: neighbours differ by > 1e-4 relative
    protos, queries = _separated_world(d, hi, rng)
    N, T = 2000, 3
    group = rng.integers(0, len(protos), size=N)
    corpus = protos[group]
    d64 = np.stack([fp64_distances(qv, protos, "l2") for qv in queries])             # [Q, prototypes]
    for row in d64:                                                                  # the separation the reference rests on (rel. 4e-5 = 2 x the
        s = np.sort(row)                                                             # schedules' distance tolerance, tie_ref.DIST_RTOL)
        assert np.all(np.diff(s) > 1e-4 * np.maximum(1.0, s[1:]))
    mt = _multi(_hashers(d, 6, T, mean=(hi - 1) / 2, spread=hi / 12 ** 0.5), corpus, id_base=-40)
    q = dev(queries)
    n_shared = n_short = 0
    for P in (1, 4):                                                                 # one probe per table: few candidates, short lists at k = 256
        cand = [[] for _ in queries]
        total = np.zeros(len(queries), np.int64)
        for table in mt.tables:
            keys, nkeys = table.hash_device(q, hash_times=P, probes="ranked")
            keys, nkeys = keys.cpu().numpy(), nkeys.cpu().numpy()
            i2r = {key: rows.cpu().numpy() for key, rows in table.index2row.items()}
            full = table._hashing.key_mode == _capi.KEY_FULL
            for qi in range(len(queries)):
                names = dict.fromkeys((int(v) & 0xFFFFFFFF) if full else int(v) for v in keys[qi, :nkeys[qi]])
                rows = [i2r[name] for name in names if name in i2r]
                mine = np.concatenate(rows) if rows else np.zeros(0, np.int64)
                assert len(np.unique(mine)) == len(mine)
                total[qi] += len(mine)
                cand[qi].append(mine)
        for k in (10, 256):
            dist, idx, ncand = mt.query_tensors(q, k=k, hash_times=P, probes="ranked")
            idx_h, nc_h = idx.cpu().numpy(), ncand.cpu().numpy()
            for qi in range(len(queries)):                                               # no query is left out
                union = np.unique(np.concatenate(cand[qi]))
                n_shared += int(total[qi] > len(union))
                n_short += int(len(union) < k)
                dd = d64[qi, group[union + 40]]                                          # id = row - 40
                want = union[np.lexsort((union & 0xFFFFFFFF, dd))][:k]                   # the sort key's low word is the id as uint32: negative ids last
                assert np.array_equal(idx_h[qi, :len(want)], want) and np.all(idx_h[qi, len(want):] == -1), (d, P, k, qi)
                assert nc_h[qi] == total[qi], (d, P, k, qi)                                 # scored pairs, with multiplicity
    assert n_shared >= 8 and n_short > 0                                             # rows were found by several tables; some lists are short


# ---------------------------------------------------------------------------------------------- T = 1
def test_one_table_is_the_single_index_in_every_word():
    from nlsh_amd.indexer import Indexer
    rng = np.random.default_rng([SEED, 1])
    N, d = 2000, 100
    corpus = _rows(None, N, d, rng)
    (h,) = _hashers(d, 6, 1)
    mt = _multi([h], corpus)
    one = Indexer(h, dev(corpus), _dist("l2"), compat=False, algo="tiled")
    for Q in (1, 5, 257):
        q = dev(_queries(None, Q, d, rng, corpus))
        for k in (1, 10, 256):
            for kw in (dict(probes="ranked", hash_times=3), dict(probes="sampled", seed=3, hash_times=4)):
                _same(mt.query_tensors(q, k=k, want_keys=True, **kw), one.query_tensors(q, k=k, want_keys=True, **kw), (Q, k, kw))


# ---------------------------------------------------------------------------------------------- query()
def test_query_lists_are_the_tensor_results_short_and_empty_ones_included():
    rng = np.random.default_rng([SEED, 2])
    N, d, k = 2000, 100, 10
    corpus = _rows(None, N, d, rng)
    near = corpus[:24] + np.float32(1e-3)
    far = (rng.standard_normal((24, d)) * 40).astype(np.float32)
    q = dev(np.concatenate([near, far]))
    n_empty = n_short = n_full = 0
    for H, P in ((16, 1), (5, 3)):                                                   # sparse tables: short and empty lists; dense ones: full lists
        mt = _multi(_hashers(d, H, 3), corpus, id_base=-5)                           # ids -5 ..: -1 is a real row id
        lists, counts = mt.query(q, k=k, hash_times=P, probes="ranked")
        _, idx, ncand, keys = mt.query_tensors(q, k=k, hash_times=P, probes="ranked", want_keys=True)
        idx_h, real = idx.cpu().numpy(), _np64(keys) != M.KEY_NONE
        assert counts == ncand.cpu().numpy().tolist() and len(lists) == len(q)
        for qi, row in enumerate(lists):
            n = int(real[qi].sum())
            assert row == idx_h[qi, :n].tolist() and all(isinstance(v, int) for v in row), qi
            n_empty += n == 0
            n_short += 0 < n < k
            n_full += n == k
            assert (n == 0) == (row == [])
    assert n_empty > 0 and n_short > 0 and n_full > 0, (n_empty, n_short, n_full)


# ---------------------------------------------------------------------------------------------- mutation
def _ids_of(table):
    return np.sort(table.gid.cpu().numpy())


def test_mutated_index_is_the_freshly_built_one():
    rng = np.random.default_rng([SEED, 4])
    N0, M1, M2, d, T = 1500, 300, 200, 100, 3
    rows = _rows(None, N0 + M1 + M2, d, rng)
    centre = rows[7]
    q = dev((centre + rng.standard_normal((40, d)) * 0.02).astype(np.float32))        # every query sits on row 7: it is in every top-k
    hashers = _hashers(d, 5, T)
    mt = _multi(hashers, rows[:N0])
    kw = dict(k=10, hash_times=3, probes="ranked")
    first = mt.query_tensors(q, **kw)[1].cpu().numpy()
    assert np.all((first == 7).any(1))
    stale = mt.row_filter(deny=[1, 2, 3])
    ids1 = mt.add(dev(rows[N0:N0 + M1]))
    assert ids1.cpu().tolist() == list(range(N0, N0 + M1)) and mt.next_id == N0 + M1 and mt.generation == 1
    gone = np.unique(np.r_[7, rng.choice(N0 + M1, size=120, replace=False)])
    assert mt.remove(gone.tolist() + [10 ** 6]) == len(gone)                           # an unknown id is ignored
    new_ids = np.arange(5000, 5000 + M2)
    gone2 = np.unique(rng.choice(np.setdiff1d(np.arange(N0 + M1), gone), size=50, replace=False))
    added, n_removed = mt.update(add=dev(rows[N0 + M1:]), add_ids=dev(new_ids.astype(np.int32)), remove=dev(gone2.astype(np.int64)))
    assert added.cpu().tolist() == new_ids.tolist() and n_removed == len(gone2) and mt.generation == 3
    kept = np.setdiff1d(np.arange(N0 + M1), np.r_[gone, gone2])
    want_ids = np.r_[kept, new_ids]
    for table in mt.tables:                                                          # one id set everywhere
        assert np.array_equal(_ids_of(table), np.sort(want_ids))
    assert mt.n_rows == len(want_ids) and mt.next_id == 5000 + M2
    fresh = _multi(hashers, np.concatenate([rows[kept], rows[N0 + M1:]]), row_ids=dev(want_ids.astype(np.int32)))
    for k in (10, 256):
        for kw2 in (dict(probes="ranked", hash_times=3), dict(probes="sampled", seed=11, hash_times=5)):
            got = mt.query_tensors(q, k=k, want_keys=True, **kw2)
            _same(got, fresh.query_tensors(q, k=k, want_keys=True, **kw2), (k, kw2))
            assert not bool((got[1] == 7).any())
    assert mt.query(q, **kw) == fresh.query(q, **kw)
    with pytest.raises(ValueError, match="stale filter"):
        mt.query_tensors(q, filter=stale, **kw)
    with pytest.raises(ValueError, match="stale filter"):
        mt.query(q, filter=stale, **kw)
    nothing, n_none = mt.update()                                                    # an empty update changes nothing
    assert nothing.numel() == 0 and n_none == 0 and mt.generation == 3
    with pytest.raises(ValueError, match="ids must be new"):                         # refused by the first table: nothing changed anywhere
        mt.add(dev(rows[:2]), ids=[int(want_ids[0]), 999999])
    for table in mt.tables:
        assert np.array_equal(_ids_of(table), np.sort(want_ids))


# ---------------------------------------------------------------------------------------------- filters
def test_denying_every_querys_nearest_row_is_the_index_without_those_rows():
    rng = np.random.default_rng([SEED, 5])
    N, d, T, base = 2000, 100, 3, -30
    corpus = _rows(None, N, d, rng)
    q = dev(_queries(None, 64, d, rng, corpus))
    hashers = _hashers(d, 6, T)
    mt = _multi(hashers, corpus, id_base=base)
    kw = dict(hash_times=4, probes="ranked")
    _, nearest, _, nearest_keys = mt.query_tensors(q, k=1, want_keys=True, **kw)
    denied = np.unique(nearest.cpu().numpy()[_np64(nearest_keys) != M.KEY_NONE])      # id -1 is a real row here: padding is told by the key
    all_ids = np.arange(N) + base
    assert len(denied) > 10
    left = np.setdiff1d(all_ids, denied)
    without = _multi(hashers, corpus[left - base], row_ids=dev(left.astype(np.int32)))
    mask = np.ones(N, bool)
    mask[denied - base] = False
    filters = {"deny": mt.row_filter(deny=denied.tolist()), "allow": mt.row_filter(allow=dev(left.astype(np.int64))), "mask": mt.row_filter(mask=dev(mask))}
    for name, F in filters.items():
        assert F.n_allowed == len(left) and len(F.filters) == T and F.generation == 0, name
        for k in (1, 10, 256):
            got = mt.query_tensors(q, k=k, filter=F, want_keys=True, **kw)
            want = without.query_tensors(q, k=k, want_keys=True, **kw)
            _same(got[:2] + got[3:], want[:2] + want[3:], (name, k))                 # ids, distance bits, sort keys
            keys_all, counts_all = _per_table(mt, q, filters=F, k=k, **kw)
            _assert_is_the_merge(got, keys_all, counts_all, k, (name, k))            # counts: the tables' own, taken before the filter
            assert not np.isin(got[1].cpu().numpy(), denied).any()
        assert mt.query(q, k=10, filter=F, **kw)[0] == without.query(q, k=10, **kw)[0], name
    other = _multi(hashers, corpus, id_base=base)
    with pytest.raises(ValueError, match="another index"):
        mt.query_tensors(q, filter=other.row_filter(deny=[0]), **kw)
    with pytest.raises(ValueError, match="single table"):
        mt.query_tensors(q, filter=mt.tables[0].row_filter(deny=[0]), **kw)


# ---------------------------------------------------------------------------------------------- strided query views
def test_strided_query_views_give_the_contiguous_results():
    rng = np.random.default_rng([SEED, 6])
    N, d, Q = 2000, 100, 37
    corpus = _rows(None, N, d, rng)
    qn = _queries(None, Q, d, rng, corpus)
    mt = _multi(_hashers(d, 6, 2), corpus)
    kw = dict(k=10, hash_times=3, probes="ranked", want_keys=True)
    want = mt.query_tensors(dev(qn), **kw)
    wide = torch.zeros((Q, d + 28), dtype=torch.float32, device="cuda")
    wide[:, :d] = dev(qn)
    every_other = torch.zeros((2 * Q, d), dtype=torch.float32, device="cuda")
    every_other[::2] = dev(qn)
    columns = torch.zeros((Q, 2 * d), dtype=torch.float32, device="cuda")
    columns[:, ::2] = dev(qn)
    for name, view in (("row pitch", wide[:, :d]), ("every other row", every_other[::2]), ("every other column", columns[:, ::2])):
        assert not view.is_contiguous()
        _same(mt.query_tensors(view, **kw), want, name)
        assert mt.query(view, k=10, hash_times=3, probes="ranked") == mt.query(dev(qn), k=10, hash_times=3, probes="ranked"), name
