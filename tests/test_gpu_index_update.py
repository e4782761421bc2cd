"""`Indexer.add` / `remove` / `update` against THE REBUILD: after any sequence of mutations every array of the index equals, word for
word, what the constructor builds from the index's rows in local order (the kept rows, then every added batch) with their ids as
`row_ids=` and their keys as `corpus_keys=`.  No tolerance anywhere.  Keys are injected (`corpus_keys=` / `keys=`), drawn from the keys
the query batch hashes to, so that the bucket layout is chosen and the queries still find candidates; rows are small integers stored as
fp32, so nothing is rounded.  The placement rule itself is held to a stable sort on the CPU (tests/test_index_update_cpu.py)."""
import numpy as np
import pytest
import torch

from helpers import dev, make_hashing
from nlsh_amd import _capi, synth

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
Q, K, P = 64, 5, 4
ALGOS = ("query", "bucket", "tiled")
ARRAYS = ("perm", "corpus_keys", "uniq_keys", "offsets", "corpus_sorted", "gid", "inv_norm")


def _dist(metric):
    from nlsh_amd.data import Glove, SIFT
    return SIFT.distance if metric == "l2" else Glove.distance


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
        assert torch.equal(_bits(a), _bits(b)), what


def assert_same_index(a, b, queries=None):
    """Every array the contract names, word for word (float arrays by their bits, padding columns included), then what is derived from
    them: `index2row`, `cells(64)`, and the results of all three schedules."""
    assert a.n_buckets == b.n_buckets and a.row_stride == b.row_stride and a.dim == b.dim
    for name in ARRAYS:
        _same(getattr(a, name), getattr(b, name), name)
    _same(a.bucket_order[:a.n_buckets], b.bucket_order[:b.n_buckets], "bucket_order")     # (one unwritten slot on an empty index)
    assert np.array_equal(a._uniq_host, b._uniq_host) and a._uniq_host.dtype == b._uniq_host.dtype
    assert np.array_equal(a._offs_host, b._offs_host) and a._offs_host.dtype == b._offs_host.dtype
    assert np.array_equal(a.bucket_sizes, b.bucket_sizes)
    ca, cb = a.cells(64), b.cells(64)
    assert ca[3] == cb[3]
    for i in range(3 if a.n_buckets else 0):      # (nothing is written for an empty index)
        _same(ca[i], cb[i], f"cells(64)[{i}]")
    ia, ib = a.index2row, b.index2row
    assert list(ia) == list(ib)
    for key in ia:
        assert torch.equal(ia[key], ib[key]), key
    if queries is None:
        return
    old = a.algo, b.algo
    try:
        for algo in ALGOS:
            a.algo = b.algo = algo
            ra = a.query_tensors(queries, k=K, hash_times=P, seed=11)
            rb = b.query_tensors(queries, k=K, hash_times=P, seed=11)
            for i, what in enumerate(("dist", "idx", "ncand")):
                _same(ra[i], rb[i], (algo, what))
    finally:
        a.algo, b.algo = old


class World:
    """One hasher, one query batch and the keys it hashes to (the pool bucket keys are drawn from), plus the rows / ids / keys an index
    under test should hold, in local order: the model every mutation is mirrored into and the rebuild is made from."""

    def __init__(self, d, metric="l2", row_align=4, seed=0):
        self.d, self.metric, self.row_align = d, metric, row_align
        self.rng = np.random.default_rng(1000 * d + seed)
        Ws, bs = synth.make_weights([d, 8, 16], seed=d)
        self.hashing = make_hashing(d, (8,), 16, Ws, bs, compat=False)
        self.queries = dev(self.rng.integers(-8, 9, size=(Q, d)).astype(np.float32))
        hard = self.hashing.hash_device(self.queries, n=1)[0].reshape(-1).cpu().numpy()
        self.pool = np.unique(np.r_[hard, np.arange(100, 100 + 8)]).astype(np.int32)     # ascending; at least 8 keys even at d = 1
        self.rows = torch.empty((0, d), dtype=torch.float32, device="cuda")
        self.ids, self.keys = np.zeros((0,), np.int32), np.zeros((0,), np.int32)

    def vectors(self, n):
        return dev(self.rng.integers(-8, 9, size=(n, self.d)).astype(np.float32))

    def indexer(self, **kw):
        from nlsh_amd.indexer import Indexer
        return Indexer(self.hashing, self.rows, _dist(self.metric), compat=False, row_align=self.row_align, **kw)

    def start(self, n, keys, row_ids=None, id_base=0):
        """The index under test, built by the constructor from n fresh rows."""
        self.rows, self.keys = self.vectors(n), np.asarray(keys, np.int32)
        self.ids = (np.arange(id_base, id_base + n) if row_ids is None else np.asarray(row_ids)).astype(np.int32)
        kw = {"id_base": id_base} if row_ids is None else {"row_ids": dev(self.ids)}
        return self.indexer(corpus_keys=dev(self.keys), **kw)

    def rebuilt(self):
        return self.indexer(corpus_keys=dev(self.keys), row_ids=dev(self.ids))

    def added(self, vectors, ids, keys):
        self.rows = torch.cat([self.rows, vectors])
        self.ids = np.r_[self.ids, ids.cpu().numpy()].astype(np.int32)
        self.keys = np.r_[self.keys, np.asarray(keys, np.int32)].astype(np.int32)

    def removed(self, ids):
        stay = ~np.isin(self.ids, ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids))
        self.rows, self.ids, self.keys = self.rows[dev(stay)], self.ids[stay], self.keys[stay]
        return int((~stay).sum())

    def add(self, ix, n, keys, **kw):
        v, keys = self.vectors(n), np.asarray(keys, np.int32)
        ids = ix.add(v, keys=dev(keys), **kw)
        assert ids.dtype == torch.int32 and ids.shape == (n,) and ids.is_cuda
        self.added(v, ids, keys)
        return ids

    def remove(self, ix, ids):
        got = ix.remove(ids)
        assert got == self.removed(ids)
        return got

    def check(self, ix, queries=True):
        assert_same_index(ix, self.rebuilt(), self.queries if queries else None)


def _spread(w, n, n_buckets):
    """n keys over the first n_buckets pool keys, every bucket hit, in a shuffled order."""
    if n == 0:
        return np.zeros((0,), np.int32)
    keys = w.pool[np.r_[np.arange(n_buckets), w.rng.integers(0, n_buckets, size=max(n - n_buckets, 0))][:n]]
    return w.rng.permutation(keys)


# ---------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("d,row_align,metric", [(1, 4, "l2"), (100, 4, "l2"), (100, 32, "cosine"), (128, 4, "cosine"), (128, 4, "l2"),
                                                (260, 4, "l2"), (260, 4, "cosine")])
@pytest.mark.parametrize("N,M", [(0, 1), (0, 300), (1, 1), (1, 64), (257, 1), (257, 64), (257, 300)])
def test_add_equals_the_rebuild(d, row_align, metric, N, M):
    w = World(d, metric, row_align, seed=N + M)
    ix = w.start(N, _spread(w, N, min(N, 5)))
    assert ix.generation == 0 and ix.next_id == N
    ids = w.add(ix, M, _spread(w, M, min(M, 7)))
    assert ids.tolist() == list(range(N, N + M)) and ix.next_id == N + M and ix.generation == 1
    assert ix._candidate_vectors_gpu is None
    w.check(ix, queries=(N, M) in ((0, 300), (257, 64), (257, 300)))


# ---------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("layout", ["below", "above", "interleaved", "existing", "one_new", "extremes_new", "extremes_both"])
def test_key_layouts(layout):
    w = World(100, "l2")
    p = w.pool
    old = p[[2, 4, 6]]
    if layout == "extremes_both":
        old = np.r_[old, I32_MIN, I32_MAX].astype(np.int32)
    ix = w.start(257, np.r_[old, w.rng.choice(old, size=257 - len(old))])
    new = {"below": p[[0, 1]], "above": p[[7]], "interleaved": p[[1, 3, 5, 7]], "existing": p[[2, 4, 6]], "one_new": p[[3]],
           "extremes_new": np.array([I32_MIN, I32_MAX, p[3]]), "extremes_both": np.array([I32_MIN, I32_MAX, I32_MIN + 1, I32_MAX - 1])}[layout]
    w.add(ix, 64, w.rng.choice(new.astype(np.int32), size=64))
    w.check(ix)
    n_buckets = len(np.unique(w.keys))
    assert ix.n_buckets == n_buckets


def test_three_buckets_grow_to_three_hundred_and_back():
    w = World(128, "l2")
    ix = w.start(257, _spread(w, 257, 3))
    assert ix.n_buckets == 3
    fresh = np.arange(5000, 5297, dtype=np.int32)                # 297 keys of their own
    ids = w.add(ix, 297, fresh)
    assert ix.n_buckets == 300
    w.check(ix)
    w.remove(ix, ids)
    assert ix.n_buckets == 3 and ix.generation == 2
    w.check(ix)


# ---------------------------------------------------------------------------------------------- removals
def test_removals():
    w = World(100, "cosine")
    ix = w.start(257, _spread(w, 257, 6), id_base=1000)
    first, last = int(ix.gid[0]), int(ix.gid[-1])
    assert w.remove(ix, [first]) == 1
    w.check(ix)
    assert w.remove(ix, torch.tensor([last], device="cuda")) == 1
    w.check(ix, queries=False)
    bucket = ix.gid[int(ix.offsets[2]):int(ix.offsets[3])].clone()          # a whole bucket, in the middle
    nb = ix.n_buckets
    assert w.remove(ix, bucket) == bucket.numel()
    assert ix.n_buckets == nb - 1
    w.check(ix)
    gen = ix.generation
    assert ix.remove([5, 6, 7]) == 0 and ix.remove([]) == 0 and ix.generation == gen      # unknown ids (id_base = 1000): nothing happens
    some = [int(ix.gid[3]), int(ix.gid[3]), int(ix.gid[9]), 999999, -4]                  # duplicates count once, unknown ids are ignored
    assert w.remove(ix, some) == 2
    w.check(ix, queries=False)
    n_left = len(w.ids)
    assert w.remove(ix, np.r_[w.ids, w.ids]) == n_left == 257 - 2 - bucket.numel() - 2    # every row
    assert ix.n_buckets == 0 and ix.gid.numel() == 0 and ix.corpus_sorted.shape == (0, ix.row_stride)
    w.check(ix)
    ids = w.add(ix, 64, _spread(w, 64, 4))                                                # ... and it fills up again
    assert int(ids[0]) == 1257                                                            # ids of removed rows are not reused
    w.check(ix)


def test_remove_and_add_in_one_update():
    w = World(128, "cosine")
    ix = w.start(257, _spread(w, 257, 5))
    gone = ix.gid[::3].clone()
    v, keys = w.vectors(64), _spread(w, 64, 8)
    ids, n_removed = ix.update(add=v, add_keys=dev(keys), remove=gone)
    assert n_removed == w.removed(gone.cpu().numpy()) == gone.numel() and ix.generation == 1
    w.added(v, ids, keys)
    assert ids.tolist() == list(range(257, 257 + 64))
    w.check(ix)
    # removal applies to the old rows only: an id added by the same call stays
    v = w.vectors(2)
    ids, n_removed = ix.update(add=v, add_ids=[7000, 7001], add_keys=dev(w.pool[:2]), remove=[7000, int(w.ids[0])])
    assert n_removed == w.removed([int(w.ids[0])]) == 1
    w.added(v, ids, w.pool[:2])
    assert ix.next_id == 7002
    w.check(ix, queries=False)


# ---------------------------------------------------------------------------------------------- ids
def test_ids():
    w = World(100, "l2")
    ix = w.start(20, _spread(w, 20, 3))
    w.remove(ix, [18, 19])
    assert w.add(ix, 2, w.pool[:2]).tolist() == [20, 21]                   # not 18, 19
    assert w.add(ix, 2, w.pool[:2], ids=dev(np.array([50, 40], np.int32))).tolist() == [50, 40] and ix.next_id == 51
    assert w.add(ix, 1, w.pool[:1], ids=[3000]).tolist() == [3000]
    assert w.add(ix, 1, w.pool[:1]).tolist() == [3001]
    w.check(ix)
    gen = ix.generation
    for bad in ([5, 5], [0, 7777], [21, 22]):                              # not distinct; in the index already
        with pytest.raises(ValueError):
            ix.add(w.vectors(2), ids=bad, keys=dev(w.pool[:2]))
    with pytest.raises(ValueError):
        ix.add(w.vectors(2), ids=[1, 2, 3], keys=dev(w.pool[:2]))
    assert ix.generation == gen
    assert ix.add(w.vectors(0)).numel() == 0 and ix.generation == gen      # M = 0: a no-op
    w.check(ix, queries=False)


def test_an_index_built_with_row_ids_requires_ids():
    w = World(128, "l2")
    given = w.rng.permutation(5000)[:257]
    ix = w.start(257, _spread(w, 257, 4), row_ids=given)
    with pytest.raises(ValueError, match="ids="):
        ix.add(w.vectors(3), keys=dev(w.pool[:3]))
    w.add(ix, 3, w.pool[:3], ids=[9001, 9000, 9002])
    w.remove(ix, given[:40])
    w.check(ix)
    assert torch.equal(ix.row_ids, dev(w.ids))                             # the id list in local order


# ---------------------------------------------------------------------------------------------- metric, strides
def test_cosine_zero_row_and_inv_norm_bits():
    w = World(100, "cosine", row_align=32)
    ix = w.start(257, _spread(w, 257, 4))
    before = {int(g): int(b) for g, b in zip(ix.gid.tolist(), ix.inv_norm.view(torch.int32).tolist())}
    v = w.vectors(64)
    v[5] = 0.0                                                             # the 1e-8 clamp
    keys = _spread(w, 64, 6)
    ids = ix.add(v, keys=dev(keys))
    w.added(v, ids, keys)
    after = {int(g): b for g, b in zip(ix.gid.tolist(), ix.inv_norm.tolist())}
    assert 9e7 < after[int(ids[5])] < 2e8                                  # 1 / 1e-8 (its bits: the rebuild's, below)
    bits = {int(g): int(b) for g, b in zip(ix.gid.tolist(), ix.inv_norm.view(torch.int32).tolist())}
    assert all(bits[g] == b for g, b in before.items())                    # old rows: copied
    w.check(ix)                                                            # new rows: the rebuild's bits


@pytest.mark.parametrize("d", [100, 127, 260])
def test_strided_views_as_vectors(d):
    w = World(d, "cosine")
    ix = w.start(257, _spread(w, 257, 4))
    wide = w.vectors(64 * 3).reshape(64, 3 * d)
    for v in (wide[:, 1:1 + d], wide[::2, d:2 * d]):                        # unaligned row starts, a row step
        keys = _spread(w, v.shape[0], 5)
        ids = ix.add(v, keys=dev(keys))
        w.added(v.contiguous(), ids, keys)
    w.check(ix)


# ---------------------------------------------------------------------------------------------- staleness
def _warm(ix, q):
    """Every cache an Indexer keeps, filled: task tables, workspaces, range plans, key tables, cells, the host directories."""
    out = []
    for algo in ALGOS:
        ix.algo = algo
        out.append(ix.query(q, k=K, hash_times=P, seed=3))
        out.append(ix.query(q, k=K, hash_times=P, probes="ranked"))
        out.append(ix.query(q, k=K, hash_times=P, probes="ranked", candidate_budget=40))
        t = ix.query_tensors(q, k=K, hash_times=P, seed=3)
        out.append((t[1].tolist(), t[2].tolist()))
    ix.algo = None
    ix.cells(64), ix.index2row, ix._size_biased_bucket()
    return out


@pytest.mark.parametrize("direction", ["grow", "shrink"])
def test_every_cache_is_dropped(direction):
    from nlsh_amd.indexer import Indexer
    w = World(128, "l2")
    old_switch = Indexer.ranked_one_call
    Indexer.ranked_one_call = True         # the ranked range plans and key tables too
    try:
        if direction == "grow":            # 3 buckets -> 303
            ix = w.start(257, _spread(w, 257, 3))
            _warm(ix, w.queries)
            w.add(ix, 300, np.arange(7000, 7300, dtype=np.int32))
            assert ix.n_buckets == 303
        else:                              # 200 buckets -> 1
            ix = w.start(300, np.r_[np.full(100, w.pool[0]), np.arange(7000, 7200)].astype(np.int32))
            _warm(ix, w.queries)
            w.remove(ix, w.ids[w.keys != w.pool[0]])
            assert ix.n_buckets == 1
        assert not ix._ws and not ix._max_tasks and not ix._cells and "_range_plans" not in ix.__dict__
        fresh = w.rebuilt()
        assert _warm(ix, w.queries) == _warm(fresh, w.queries)
        assert_same_index(ix, fresh, w.queries)
    finally:
        Indexer.ranked_one_call = old_switch


def test_a_pipeline_built_before_a_mutation_raises_on_submit():
    from nlsh_amd.pipeline import QueryPipeline
    w = World(128, "l2")
    ix = w.start(257, _spread(w, 257, 3))
    pipe = QueryPipeline(ix, w.queries, k=K, hash_times=P, depth=2)
    pipe.submit(w.queries, seed=5)
    pipe.synchronize()
    w.add(ix, 300, np.arange(7000, 7300, dtype=np.int32))
    with pytest.raises(_capi.NlshHipError, match="generation 0.*generation 1") as e:
        pipe.submit(w.queries, seed=5)
    assert e.value.code == _capi.E_INVALID
    pipe.close()
    pipe = QueryPipeline(ix, w.queries, k=K, hash_times=P, depth=2)
    dist, idx, ncand, _ = pipe.submit(w.queries, seed=5)
    pipe.synchronize()
    want = w.rebuilt().query_tensors(w.queries, k=K, hash_times=P, seed=5)
    for got, ref, what in zip((dist, idx, ncand), want, ("dist", "idx", "ncand")):
        _same(got, ref, what)
    pipe.close()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.hashings import MultivariateBernoulli
    from nlsh_amd.indexer import Indexer
    w = World(100, "l2")
    ix = w.start(20, _spread(w, 20, 3))
    keys = dev(w.pool[:2])
    with pytest.raises(_capi.NlshHipError) as e:
        ix.add(torch.zeros(2, 100), keys=keys)                              # a host tensor
    assert e.value.code == _capi.E_INVALID and "no CPU path" in str(e.value)
    with pytest.raises(ValueError):
        ix.add(torch.zeros(2, 101, device="cuda"), keys=keys)               # wrong d
    with pytest.raises(ValueError):
        ix.add(torch.zeros(2, 100, device="cuda", dtype=torch.float64), keys=keys)
    with pytest.raises(ValueError):
        ix.add(torch.zeros(2, 100, device="cuda"), keys=keys.long())        # keys: int32
    with pytest.raises(ValueError):
        ix.remove(torch.tensor([1.5], device="cuda"))
    assert ix.generation == 0
    w.check(ix, queries=False)

    generic = Indexer(w.hashing, w.rows, lambda a, b: (a - b).abs().sum(-1), compat=False, corpus_keys=dev(w.keys))
    for call in (lambda: generic.add(w.vectors(2), keys=keys), lambda: generic.remove([0]), lambda: generic.update(remove=[0])):
        with pytest.raises(NotImplementedError):
            call()

    bn = MultivariateBernoulli(MultiLayerRelu(100, [8], with_batchnorm=True), 16, None, compat=False)
    bn.train_mode(False)
    ixb = Indexer(bn, w.rows, _dist("l2"), compat=False)
    bn.train_mode(True)
    with pytest.raises(_capi.NlshHipError) as e:
        ixb.add(w.vectors(4))
    assert e.value.code == _capi.E_UNSUPPORTED and ixb.generation == 0
    assert ixb.add(w.vectors(4), keys=dev(w.pool[:4])).tolist() == [20, 21, 22, 23]     # keys given: nothing is hashed
    bn.train_mode(False)


# ---------------------------------------------------------------------------------------------- a medium index, a real hasher
def test_ten_mutations_of_a_20000_row_index_with_hashed_keys():
    from nlsh_amd.indexer import Indexer
    N, d = 20000, 128
    rng = np.random.default_rng(5)
    Ws, bs = synth.make_weights([d, 64, 12], seed=9)
    hashing = make_hashing(d, (64,), 12, Ws, bs, compat=False)
    vec = lambda n: dev(rng.integers(-8, 9, size=(n, d)).astype(np.float32))   # noqa: E731
    rows, ids = vec(N), np.arange(N, dtype=np.int32)
    ix = Indexer(hashing, rows, _dist("l2"), compat=False)
    for step in range(10):
        kind = ("add", "remove", "both", "add", "remove")[step % 5]
        gone = rng.choice(ids, size=int(rng.integers(1, 2000)), replace=False) if kind != "add" else None
        v = vec(int(rng.integers(1, 3000))) if kind != "remove" else None
        new_ids, n_removed = ix.update(add=v, remove=None if gone is None else dev(gone))
        if gone is not None:
            assert n_removed == len(gone)
            stay = ~np.isin(ids, gone)
            rows, ids = rows[dev(stay)], ids[stay]
        if v is not None:
            rows, ids = torch.cat([rows, v]), np.r_[ids, new_ids.cpu().numpy()].astype(np.int32)
    assert ix.generation == 10
    fresh = Indexer(hashing, rows, _dist("l2"), compat=False, row_ids=dev(ids))     # hashes every surviving row again
    queries = vec(512)
    assert_same_index(ix, fresh, queries)
    assert ix.query(queries, k=10, hash_times=8, seed=2) == fresh.query(queries, k=10, hash_times=8, seed=2)
