"""The mass-tie reference (tests/tie_ref.py) held to the CPU oracle, and the preconditions of the GPU tie tests (tests/test_gpu_tie_order.py,
tests/test_gpu_merge_topk_ref.py) checked where no GPU is needed: the separation of the prototypes for every query of every data set,
the kinds of cut and the merge forms the key lists reach, the merge reference on hand-written keys."""
import numpy as np
import pytest

import tie_ref as T
from oracle import oracle

CPU_K = (1, 10, 33, 64, 65, 129, 256)
DATASETS = ("main", "lists", "one")


@pytest.mark.parametrize("name", DATASETS)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_prototypes_are_separated_for_every_query(metric, name):
    data = T.dataset(metric, name)
    assert data.queries.shape == (T.N_QUERIES, T.DIM[metric])
    assert np.array_equal(data.corpus, data.prototypes[data.group_of_row])          # every row an exact copy
    assert T.separation(data.queries, data.prototypes, metric) >= T.SEPARATION
    assert T.SEPARATION >= 2.5 * 2 * T.DIST_RTOL
    if name != "one":                                                               # small tie groups next to those of hundreds of rows
        sizes = np.bincount(data.group_of_row)
        assert sizes[T.N_BIG_GROUPS:].tolist() == list(T.SMALL_GROUPS) and sizes[:T.N_BIG_GROUPS].min() >= 100
        for g in range(len(sizes)):                                                 # ... whose ids are scattered, not runs
            rows = np.nonzero(data.group_of_row == g)[0]
            assert len(rows) < 4 or np.diff(rows).max() > 1


@pytest.mark.parametrize("k", CPU_K)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_expected_topk_is_the_oracles_order(metric, k):
    data = T.dataset(metric, "main")
    key_lists = T.key_lists_of(data, k)
    rows = T.candidate_rows(data.corpus_keys, key_lists)
    want, d64, ncand = T.expected_topk(data.queries, data.prototypes, data.group_of_row, np.arange(data.N), rows, k, metric)
    perm, uniq, offs = oracle.build_csr(data.corpus_keys.astype(np.int64))
    qk, nk = oracle.keys_from_lists([list(dict.fromkeys(ks)) for ks in key_lists])
    od, oi, onc = oracle.query_batch(data.corpus, perm, uniq, offs, data.queries, qk, nk, k, metric)
    assert np.array_equal(onc, ncand)
    assert np.array_equal(oi, want)
    ok = want >= 0
    assert np.all(np.isposinf(od[~ok])) and np.all(np.abs(od[ok] - d64[ok]) <= T.DIST_RTOL * np.maximum(1.0, np.abs(d64[ok])))
    groups = np.where(ok, data.group_of_row[np.maximum(want, 0)], -1)
    bits = od.view(np.uint32)
    for q in range(T.N_QUERIES):                                                    # one tie group, one bit pattern
        for g in np.unique(groups[q][ok[q]]):
            assert len(np.unique(bits[q][groups[q] == g])) == 1, (q, g)


@pytest.mark.parametrize("k", T.ALL_K)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_every_kind_of_cut_is_present(metric, k):
    data = T.dataset(metric, "main")
    key_lists = T.key_lists_of(data, k)
    assert any(len(ks) == 1 for ks in key_lists) and any(2 <= len(ks) <= 4 for ks in key_lists)     # one bucket, a few,
    assert max(len(set(ks)) for ks in key_lists) == 55                                              # all of them
    pd = T.prototype_distances(data.queries, data.prototypes, metric)
    seen = set()
    for q, rows in enumerate(T.candidate_rows(data.corpus_keys, key_lists)):
        seen |= T.cut_classes(pd[q], data.group_of_row[rows], k)
    assert seen == {"inside", "group_end", "exact", "short", "one_group"}
    if k <= 64:
        for name in ("lists", "one"):
            other = T.dataset(metric, name)
            opd = T.prototype_distances(other.queries, other.prototypes, metric)
            kinds = set()
            for q, rows in enumerate(T.candidate_rows(other.corpus_keys, T.key_lists_of(other, k))):
                kinds |= T.cut_classes(opd[q], other.group_of_row[rows], k)
            assert "inside" in kinds


@pytest.mark.parametrize("k", T.NARROW_K)
def test_list_counts_cover_every_merge_form(k):
    """merge_query at 64 rows per list (seg_rows = 64, the wave-level bucket-major schedule): one key per lane, two, one general round,
    several rounds, the untabbed search (more than 128 lists; a probe of more than 8 segments)."""
    data = T.dataset("l2", "lists")
    assert T.dataset("cosine", "lists").bucket_rows == data.bucket_rows
    seen = set()
    for L, widest in T.list_counts(data.bucket_rows, T.key_lists_of(data, k), 64):
        seen |= T.merge_classes(L, widest, k)
    assert seen == {"le_R", "le_2R", "one_round", "rounds", "gt_128", "probe_gt_8"}
    # the query-major schedule cuts a query's whole candidate list into segments: a dozen and more partial lists per query
    assert max(L for L, _ in T.list_counts(data.bucket_rows, T.key_lists_of(data, k), 64)) >= 12


def test_tiled_list_counts_on_the_main_layout():
    """256 rows per list (the tiled schedule): the 2100-row bucket is 9 segments -- the untabbed search of merge_query and
    merge_query_wide --, the wide merges see one list, one round of three (k <= 128) and several rounds."""
    data = T.dataset("l2", "main")
    for k in T.ALL_K:
        counts = T.list_counts(data.bucket_rows, T.key_lists_of(data, k), 256)
        assert max(w for _, w in counts) == 9
        Ls = {L for L, _ in counts}
        assert 1 in Ls and 2 in Ls and 3 in Ls and max(Ls) > 12 and any(w <= 8 and L > 3 for L, w in counts)


def _keys(pairs):
    return T.make_keys(np.array([p[0] for p in pairs], np.float32), [p[1] for p in pairs])


def test_merge_reference_on_hand_written_keys():
    big = 2 ** 31 - 1
    tiny = np.float32(1e-45)                                                         # a denormal
    one_up = np.nextafter(np.float32(1), np.float32(2))
    lists = [
        [(-np.inf, 7), (-1.0, 3), (-0.0, 9), (0.0, 2), (1.0, big), (np.inf, 0)],
        [(-tiny, 4), (0.0, 1), (tiny, 5), (1.0, 0), (one_up, 6), (np.inf, big)],
    ]
    keys_in = np.stack([_keys(lst) for lst in lists])[:, None, :]                    # [G = 2, Q = 1, 6]
    assert np.all(np.diff(keys_in[:, 0, :].astype(object), axis=1) > 0)              # each list ascending as uint64
    dist, idx = T.merge_reference(keys_in, 6)
    want = [(-np.inf, 7), (-1.0, 3), (-tiny, 4), (-0.0, 9), (0.0, 1), (0.0, 2)]      # -0.0 sorts before +0.0: different distance words
    assert idx[0].tolist() == [p[1] for p in want]
    assert np.array_equal(dist[0].view(np.uint32), np.array([p[0] for p in want], np.float32).view(np.uint32))
    dist, idx = T.merge_reference(keys_in, 5)                                        # only the first k of each list are read
    assert idx[0].tolist() == [7, 3, 4, 9, 1]
    full = np.concatenate([keys_in, np.full((1, 1, 6), T.KEY_NONE)])                 # an empty list; fewer than k real keys
    dist, idx = T.merge_reference(np.pad(full, ((0, 0), (0, 0), (0, 9)), constant_values=T.KEY_NONE), 15)
    assert idx[0].tolist() == [7, 3, 4, 9, 1, 2, 5, 0, big, 6, 0, big, -1, -1, -1]
    assert np.array_equal(dist[0, 6:12], np.array([tiny, 1.0, 1.0, one_up, np.inf, np.inf], np.float32))
    assert np.all(np.isposinf(dist[0, 12:]))
    m = T.mono_from_float(np.array([-np.inf, -1.0, -tiny, -0.0, 0.0, tiny, 1.0, one_up, np.inf], np.float32))
    assert np.all(np.diff(m.astype(np.int64)) > 0) and int(m[7]) - int(m[6]) == 1 and int(m[4]) - int(m[3]) == 1
    assert np.array_equal(T.float_from_mono(m).view(np.uint32),
                          np.array([-np.inf, -1.0, -tiny, -0.0, 0.0, tiny, 1.0, one_up, np.inf], np.float32).view(np.uint32))
