"""`Indexer.query()` with its results stored to pinned host memory by the merge kernel itself (`nlsh_query_batch_host`, bmerge_host_kernel):
the lists equal those built from `hash_device` + `scan_tensors` + the facade's F7 rule on the same seed (the comparison of
tools/fuzz_parity.py), only the short queries' key rows are written, the overflow retry is driven by the status words of the host
block, and the export refuses what it cannot serve before anything is enqueued.

Small indexes with a random-init hash: most buckets are tiny or missing, so queries with fewer than k candidates (the F7 rule's
cases) and with none at all are plentiful."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import dev, make_hashing

pytestmark = pytest.mark.gpu

N, K = 3000, 10
POISON = 0x5A5A5A5A          # no id (< 3000), count (<= 3000 * P), status word or key (< 2^24) of these cases equals it
# (d, H, compat keys, metric): H = 16 with the reference's int16 keys, H = 24 with full-width keys, each under both metrics
INDEXES = {"d24_h16_l2": (24, 16, True, "l2"), "d100_h24_cos": (100, 24, False, "cosine"),
           "d100_h16_cos": (100, 16, True, "cosine"), "d24_h24_l2": (24, 24, False, "l2"),
           # full-width keys on at most 1,024 buckets, most of them populated: queries with k candidates or more beside short ones with real ids
           # in front of the -1 padding -- the non-compat branch (ids >= 0 filtered from the host block) on lists that are not empty
           "d24_h10_full_l2": (24, 10, False, "l2")}
SPARSE = ("h16", "h24")      # the indexes of tiny or missing buckets: empty AND short queries in every batch of 257 or more
_built, _queries, _reference = {}, {}, {}


def _index(name):
    if name not in _built:
        from nlsh_amd import synth
        from nlsh_amd.data import Glove, SIFT
        from nlsh_amd.indexer import Indexer
        d, H, compat, metric = INDEXES[name]
        gen = synth.sift_like if metric == "l2" else synth.glove_like
        corpus = gen(N, d, seed=311)
        mean = std = None
        if metric == "l2":
            corpus, mean, std = synth.standardise(corpus)
        Ws, bs = synth.make_weights([d, 64, H], seed=313)
        hashing = make_hashing(d, [64], H, Ws, bs, compat=compat, seed=7)
        ix = Indexer(hashing, dev(corpus), SIFT.distance if metric == "l2" else Glove.distance, compat=compat)
        _built[name] = (ix, gen, mean, std, d)
    return _built[name]


def _batch(name, Q):
    if (name, Q) not in _queries:
        from nlsh_amd import synth
        ix, gen, mean, std, d = _index(name)
        q = gen(Q, d, seed=317 + Q)
        if mean is not None:
            q = synth.standardise(q, mean, std)[0]
        _queries[(name, Q)] = dev(q)
    return _queries[(name, Q)]


def _expected(name, Q, P, seed, algo=None):
    """(lists, counts, counts array, keys, nkeys) from the device-resident calls and the facade's F7 rule; computed once per case."""
    key = (name, Q, P, seed, algo)
    if key not in _reference:
        from nlsh_amd.hashings import host_key_set
        ix = _index(name)[0]
        q = _batch(name, Q)
        ix.algo = algo
        keys, nkeys = ix.hash_device(q, hash_times=P, seed=seed)
        _, idx, nc, _ = ix.scan_tensors(q, keys, nkeys, k=K)
        idx, nc, kh, nkh = idx.cpu().numpy(), nc.cpu().numpy(), keys.cpu().numpy(), nkeys.cpu().numpy()
        lists = []
        for i in range(Q):
            if nc[i] >= K:
                lists.append(idx[i].tolist())
            elif not ix.compat:
                lists.append([int(v) for v in idx[i] if v >= 0])
            else:
                ks = list(host_key_set(kh[i], int(nkh[i]), ix._hashing.key_mode))
                lists.append(ix._rows_of_key(ks[-1]) if ks else [])
        _reference[key] = (lists, nc.tolist(), nc, kh, nkh)
    return _reference[key]


def _query(name, Q, P, seed, algo=None):
    ix = _index(name)[0]
    ix.algo = algo
    return ix.query(_batch(name, Q), k=K, hash_times=P, seed=seed)


@pytest.mark.parametrize("name", list(INDEXES))
@pytest.mark.parametrize("P", [1, 10])
@pytest.mark.parametrize("Q", [1, 5, 257, 4100])
def test_query_lists_equal_the_device_resident_results(name, Q, P):
    """Q = 4100 takes the two-range path (`_CHUNK_MIN_ROWS` = 2048); Q = 1 and 5 stay below 64 (query, probe) pairs, where the facade
    picks the query-major schedule and keeps its copies -- they are run on the forced tiled schedule as well, where the last workgroup
    of the host-writing merge holds fewer than four queries."""
    for algo in ((None, "tiled") if Q * P < 64 else (None,)):
        lists, counts, nc, _, _ = _expected(name, Q, P, 40 + P, algo)
        got_lists, got_counts = _query(name, Q, P, 40 + P, algo)
        assert got_counts == counts
        assert got_lists == lists
        if Q >= 257 and name == "d24_h10_full_l2":      # both kinds of list the sparse indexes hardly have: short WITH ids, and full
            assert int((nc >= K).sum()) >= 1 and int(((nc > 0) & (nc < K)).sum()) >= 1
        if Q >= 257 and any(tag in name for tag in SPARSE):
            assert int((nc == 0).sum()) >= 1 and int(((nc > 0) & (nc < K)).sum()) >= 1      # empty and short queries are both present


def _blocks(ix, Q, P):
    """[(first query, rows, offset of the range's block in the pinned buffer)] as `Indexer.query` lays them out."""
    if ix._n_chunks() > 1 and Q >= ix._n_chunks() * ix._CHUNK_MIN_ROWS:
        n = ix._n_chunks()
        bounds = [(Q * c // n, Q * (c + 1) // n) for c in range(n)]
        per = max(hi - lo for lo, hi in bounds)
        words = (per * K + per + 2 + per * P + per + 3) // 4 * 4
        return [(lo, hi - lo, c * words) for c, (lo, hi) in enumerate(bounds)]
    return [(0, Q, 0)]


@pytest.mark.parametrize("name", ["d24_h16_l2", "d100_h24_cos", "d24_h10_full_l2"])
@pytest.mark.parametrize("Q", [257, 4100])
def test_only_the_short_queries_key_rows_are_written(name, Q):
    P, seed = 10, 50
    ix = _index(name)[0]
    lists, counts, nc, keys, nkeys = _expected(name, Q, P, seed)
    assert _query(name, Q, P, seed)[0] == lists                # sizes the pinned block and the task tables: the next call makes no retry
    ix._pin.fill_(POISON)
    got = _query(name, Q, P, seed)
    assert got[0] == lists and got[1] == counts
    host = ix._pin.numpy()
    short = 0
    for lo, m, base in _blocks(ix, Q, P):
        n = m * K + m + 2
        assert not (host[base:base + n] == POISON).any()       # ids, counts and status: every word written
        assert host[base + m * K:base + m * K + m].tolist() == counts[lo:lo + m]
        rows = host[base + n:base + n + m * (P + 1)].reshape(m, P + 1)
        for i in range(m):
            if nc[lo + i] < K:
                nk = int(nkeys[lo + i])
                assert rows[i, 0] == nk and rows[i, 1:1 + nk].tolist() == keys[lo + i, :nk].tolist()
                short += 1
            else:
                assert (rows[i] == POISON).all()               # a query with >= k candidates leaves its row alone
    assert short == int((nc < K).sum()) > 0
    if name != "d100_h24_cos":
        assert short < Q                                       # ... and these indexes have queries with k candidates or more: rows left alone were seen


@pytest.mark.parametrize("Q", [257, 4100])
def test_overflow_retry_reads_the_status_words_of_the_host_block(Q):
    name, P, seed = "d24_h16_l2", 10, 60
    ix = _index(name)[0]
    lists, counts = _expected(name, Q, P, seed)[:2]
    assert _query(name, Q, P, seed)[0] == lists
    ix._max_tasks = {key: 1 for key in ix._max_tasks}          # every kept descriptor now names a one-entry task table
    got = _query(name, Q, P, seed)
    assert got[0] == lists and got[1] == counts
    rows = {m for _, m, _ in _blocks(ix, Q, P)}
    assert min(v for key, v in ix._max_tasks.items() if key[1] in rows and key[2] == P) > 1


def test_the_export_refuses_bad_result_blocks_before_anything_is_enqueued():
    from nlsh_amd import _capi
    name, Q, P, seed = "d24_h16_l2", 257, 10, 70
    ix = _index(name)[0]
    lists, counts = _expected(name, Q, P, seed)[:2]
    assert _query(name, Q, P, seed)[0] == lists
    L = _capi.lib()
    plan = next(p for p in ix._range_plans.values() if p["host_ptr"] == ix._pin.data_ptr() and p["desc"].Q == Q and p["desc"].n_probes == P)
    q = _batch(name, Q)
    need = Q * K + Q + 2 + Q * (P + 1)
    assert plan["host_words"] == need
    on_device = torch.full((need,), POISON, dtype=torch.int32, device=q.device)
    wide = _capi.StepDesc.from_buffer_copy(plan["desc"])
    wide.k = 65
    ix._pin.fill_(POISON)
    torch.cuda.synchronize()

    def call(desc, out, words):
        return L.nlsh_query_batch_host(ctypes.byref(desc), ctypes.sizeof(desc), q.data_ptr(), q.stride(0), seed, 0, 0, out, words, plan["stream"])

    for desc, out, words, word in ((plan["desc"], on_device.data_ptr(), need, b"mapped"), (plan["desc"], plan["host_ptr"], need - 1, b"words"),
                                   (wide, plan["host_ptr"], need + Q * 55, b"k=65")):
        assert call(desc, out, words) == _capi.E_INVALID
        assert word in L.nlsh_last_error(), L.nlsh_last_error()
    torch.cuda.synchronize()
    assert bool((on_device == POISON).all()) and bool((ix._pin == POISON).all())       # nothing ran: the outputs are untouched
    got = _query(name, Q, P, seed)
    assert got[0] == lists and got[1] == counts
