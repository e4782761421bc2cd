"""The route ladder of `Indexer.query()` / `query_tensors()` on the GPU: which form serves which call, and that the list form and the
tensor form of one call agree on every route, on a single row range and on two.

Nothing here is a recording of the code under test.  The expected `last_query_path` of a case is the one the docstrings of `query`,
`query_tensors`, `_fuses`, `_fuses_ranked` and of the class attribute give for it; the expected lists of `query()` are the rows of
`query_tensors()`' `idx` cut to each query's length (with the reference's short-query rule on top under compat=True, worked out here
from the corpus keys); and the unfiltered calls are held against `query_with_keys` on the key sets `hash_device` returns for the same
seed and mode, a path that shares only the key-list packer with them -- which the last test pins against the range call and numpy."""
import contextlib
import functools

import numpy as np
import pytest

from helpers import dev, make_hashing

pytestmark = pytest.mark.gpu

N, D, H, K, P, SEED = 6000, 24, 8, 5, 3, 4242
SINGLE, CHUNKED = 130, 4100             # one row range; two (query_chunks = 2 and >= 2,048 rows per range)


@contextlib.contextmanager
def one_call(on):
    from nlsh_amd.indexer import Indexer
    old = Indexer.ranked_one_call
    Indexer.ranked_one_call = on
    try:
        yield
    finally:
        Indexer.ranked_one_call = old


@functools.lru_cache(maxsize=None)
def world(kind, compat=False):
    """(indexer, corpus keys on the host) -- "plain": nothing but rows; "refine": built with refine="device" and tags= (row r: bit r % 4)."""
    from nlsh_amd import synth
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    Ws, bs = synth.make_weights([D, 32, H], seed=3, gain=3.0)
    h = make_hashing(D, [32], H, Ws, bs, compat=compat)
    rows = dev(np.random.default_rng(41).standard_normal((N, D)).astype(np.float32))
    extra = dict(refine="device", tags=dev(np.int64(1) << (np.arange(N, dtype=np.int64) % 4))) if kind == "refine" else {}
    ix = Indexer(h, rows, SIFT.distance, compat=compat, **extra)
    ix.query_chunks = 2
    return ix, ix.corpus_keys.cpu().numpy()


@functools.lru_cache(maxsize=None)
def queries(Q):
    return dev(np.random.default_rng(7 + Q).standard_normal((Q, D)).astype(np.float32))


# name -> (keywords of the call, ranked_one_call, path after query(), path after query_tensors())
RANKED = dict(probes="ranked")
BUDGET = dict(probes="ranked", candidate_budget=200)
UNFILTERED = {
    "plain": ({}, False, "fused", "fused"),
    "ranked": (RANKED, False, "two_step", "two_step"),
    "ranked+budget": (BUDGET, False, "two_step", "two_step"),
    "one_call": (RANKED, True, "ranked_one_call", "ranked_one_call"),
    "one_call+budget": (BUDGET, True, "ranked_one_call", "ranked_one_call"),
}


def key_sets_of(ix, q, kw):
    from nlsh_amd.hashings import keys_to_sets
    keys, nkeys = ix.hash_device(q, hash_times=P, seed=SEED, **kw)
    return keys_to_sets(keys, nkeys, ix._hashing.key_mode)


def expected_lists(ix, corpus_keys, idx, ncand, key_sets):
    """`query()`'s lists from the tensor form: a row without its -1 padding; `key_sets` (an unfiltered call under compat=True): a query
    with fewer than k candidates gets the rows of the last key of its set, ascending, [] for a key without a bucket."""
    out = []
    for qi, row in enumerate(idx.cpu().tolist()):
        if key_sets is not None and ncand[qi] < K:
            order = list(key_sets[qi])
            out.append(np.nonzero(corpus_keys == order[-1])[0].tolist() if order else [])
        else:
            out.append([v for v in row if v >= 0])
    return out


def both_forms(ix, corpus_keys, q, kw, on, path_lists, path_tensors, key_sets=None, ranges=None):
    """One case: (a) the paths, (b) `query()` against `query_tensors()`.  `ranges`: the rows of the last launch of a `query()` that went
    through the row ranges (the whole batch, or half of it)."""
    with one_call(on):
        lists, counts = ix.query(q, k=K, hash_times=P, seed=SEED, **kw)
        assert ix.last_query_path == path_lists, (kw, ix.last_query_path)
        if ranges is not None:
            assert ix._last_tkey[1] == ranges, (kw, ix._last_tkey)
        _, idx, ncand, _ = ix.query_tensors(q, k=K, hash_times=P, seed=SEED, **kw)
        assert ix.last_query_path == path_tensors, (kw, ix.last_query_path)
    ncand = ncand.cpu().tolist()
    assert counts == ncand, kw
    want = expected_lists(ix, corpus_keys, idx, ncand, key_sets)
    assert len(lists) == q.shape[0] and lists == want, (kw, [qi for qi, (a, b) in enumerate(zip(lists, want)) if a != b][:4])
    return lists, counts


@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("Q", [SINGLE, CHUNKED])
def test_unfiltered_routes(Q, compat):
    ix, corpus_keys = world("plain", compat)
    q = queries(Q)
    for name, (kw, on, path_lists, path_tensors) in UNFILTERED.items():
        sets = key_sets_of(ix, q, kw)
        lists, counts = both_forms(ix, corpus_keys, q, kw, on, path_lists, path_tensors, sets if compat else None,
                                   Q // 2 if Q == CHUNKED else Q)
        # (c) the same candidate sets through `query_with_keys`
        by_keys = ix.query_with_keys(q, [list(s) for s in sets], k=K)
        assert (lists, counts) == by_keys[:2], name
    if Q == CHUNKED and not compat:     # a result kept back and the one-shot conversion take the other consumer of the row ranges
        want = ix.query(q, k=K, hash_times=P, seed=SEED)
        ix.defer_result_release = True
        try:
            assert ix._shells(Q, K) is None and ix.query(q, k=K, hash_times=P, seed=SEED) == want
            ix.query_chunks = 1
            assert ix.query(q, k=K, hash_times=P, seed=SEED) == want and ix._last_tkey[1] == Q
        finally:
            ix.defer_result_release, ix.query_chunks = False, 2
            ix._keep(None)


@pytest.mark.parametrize("Q", [SINGLE, CHUNKED])
def test_filtered_tagged_and_refined_routes(Q):
    q = queries(Q)
    ix, corpus_keys = world("plain")
    deny = ix.row_filter(deny=list(range(0, N, 3)))
    lists, _ = both_forms(ix, corpus_keys, q, dict(filter=deny), False, "two_step", "two_step")
    assert all(v % 3 for row in lists for v in row) and any(lists)
    rx, rkeys = world("refine")
    lists, _ = both_forms(rx, rkeys, q, dict(tag_mask=0b0101, refine_k=0), False, "two_step", "two_step")
    assert all(v % 4 in (0, 2) for row in lists for v in row) and any(lists)
    both_forms(rx, rkeys, q, dict(tag_mask=0b0101), False, "two_step+refine", "two_step+refine")
    # the re-rank behind the form that served stage one: `query()` takes the two-step route's key table, `query_tensors()` the fused call
    both_forms(rx, rkeys, q, dict(refine_k=None), False, "two_step+refine", "fused+refine")
    both_forms(rx, rkeys, q, dict(refine_k=0), False, "fused", "fused", ranges=Q // 2 if Q == CHUNKED else Q)


def test_key_lists_are_packed_alike_for_topk_and_range_calls():
    """(d) a repeated key, a key >= 2^31 (no bucket has it) and an empty list through `query_with_keys` and `range_query_with_keys`."""
    ix, corpus_keys = world("plain")
    sizes = np.bincount(corpus_keys.astype(np.int64), minlength=1 << H)         # an 8-bit hash: the keys are 0..255
    big, small = (int(v) for v in np.argsort(sizes, kind="stable")[[-1, -2]])
    few = np.nonzero((sizes > 0) & (sizes <= K))[0]
    tiny = int(few[0]) if len(few) else small                                   # a bucket of at most k rows, where the index has one
    key_lists = [[big, small, big], [(1 << 31) + 5, small], [], [tiny], [small, (1 << 32) - 1, small, tiny]]
    q = queries(SINGLE)[:len(key_lists)]
    want_counts = [int(sum(sizes[key] for key in set(ks) if key < 1 << H)) for ks in key_lists]
    lists, counts, _, _ = ix.query_with_keys(q, key_lists, k=K)
    in_range, range_counts = ix.range_query_with_keys(q, key_lists, float("inf"))
    assert counts == range_counts == want_counts
    assert [len(r) for r in in_range] == want_counts
    for got, every, n in zip(lists, in_range, want_counts):
        assert got == every[:K]
        if n <= K:
            assert got == every
    assert lists[2] == [] and want_counts[0] > K
