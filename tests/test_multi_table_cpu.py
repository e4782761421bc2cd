"""Multi-table indexes, the parts that need no device: the new export and its host-side argument checks, the facade's refusals (all
raised before a device is touched), and the numpy reference of the unique merge held against the definition it serves."""
import ctypes
import os
import re

import numpy as np
import pytest

import multi_table_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_export_is_declared_and_present():
    from nlsh_amd import _capi
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    assert re.search(r"\bnlsh_merge_topk_unique\s*\(", header)
    assert "nlsh_merge_topk_unique" in _capi.SYMBOLS and hasattr(L, "nlsh_merge_topk_unique")
    assert re.search(r"#define NLSH_MAX_TABLES 16\b", header) and _capi.MAX_TABLES == 16
    assert re.search(r"#define NLSH_ABI_VERSION 4\b", header) and L.nlsh_abi_version() == 4      # no struct changed: no new ABI
    makefile = open(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "csrc", "Makefile")).read()
    assert "merge_unique.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, re.M).group(1)
    assert len(L.nlsh_merge_topk_unique.argtypes) == 11


def _call(L, keys_in="buf", row_stride=10, G=2, Q=1, k=10, out_dist="buf", out_idx="buf"):
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    pick = lambda v: a if v == "buf" else v
    return L.nlsh_merge_topk_unique(pick(keys_in), row_stride, G, Q, k, None, pick(out_dist), pick(out_idx), None, None, None)


@pytest.mark.parametrize("kw, code, names", [
    (dict(keys_in=None), "E_INVALID", [b"keys_in"]),
    (dict(out_dist=None), "E_INVALID", [b"out_dist"]),
    (dict(out_idx=None), "E_INVALID", [b"out_idx"]),
    (dict(G=0), "E_INVALID", [b"G=0"]),
    (dict(G=17), "E_UNSUPPORTED", [b"G=17", b"16"]),
    (dict(k=0, row_stride=10), "E_INVALID", [b"k=0"]),
    (dict(k=257, row_stride=300), "E_UNSUPPORTED", [b"k=257", b"256"]),
    (dict(k=10, row_stride=9), "E_INVALID", [b"row_stride=9"]),
    (dict(Q=-1), "E_INVALID", [b"Q=-1"]),
])
def test_merge_topk_unique_refuses_on_the_host(kw, code, names):
    """Every refusal comes from the host-side checks -- this machine has no device to touch -- and names the argument."""
    from nlsh_amd import _capi
    L = _capi.lib()
    assert _call(L, **kw) == getattr(_capi, code), (kw, L.nlsh_last_error())
    msg = L.nlsh_last_error()
    assert msg.startswith(b"merge_topk_unique:") and all(n in msg for n in names), msg


def test_merge_topk_unique_takes_an_empty_batch_and_every_k_and_G_in_range():
    from nlsh_amd import _capi
    L = _capi.lib()
    for k in (1, 64, 65, 256):
        for G in (1, 16):
            assert L.nlsh_merge_topk_unique(None, k, G, 0, k, None, None, None, None, None, None) == _capi.OK, (k, G, L.nlsh_last_error())
    assert _call(L, Q=0, G=17) == _capi.E_UNSUPPORTED          # the limits hold on an empty batch too


# ----------------------------------------------------------------------------------------------- facade refusals, no device
class _Hasher:
    pass


def _l2():
    from nlsh_amd.data import SIFT
    return SIFT.distance


def test_constructor_refuses_bad_hasher_lists_before_touching_the_corpus():
    """The corpus argument is an object() here: a constructor that reached a table's build would fail on it with another error."""
    from nlsh_amd.multitable import MultiTableIndexer
    corpus = object()
    with pytest.raises(ValueError, match="hashings is empty"):
        MultiTableIndexer([], corpus, _l2())
    with pytest.raises(ValueError, match="17 hashers.*at most 16"):
        MultiTableIndexer([_Hasher() for _ in range(17)], corpus, _l2())
    h = _Hasher()
    with pytest.raises(ValueError, match=r"hashings\[0\] and hashings\[2\] are the same object"):
        MultiTableIndexer([h, _Hasher(), h], corpus, _l2())
    with pytest.raises(ValueError, match="one key tensor per table"):
        MultiTableIndexer([_Hasher(), _Hasher()], corpus, _l2(), corpus_keys=[None])
    with pytest.raises(ValueError, match="storage must be"):
        MultiTableIndexer([_Hasher()], corpus, _l2(), storage="int4")
    with pytest.raises(NotImplementedError, match="'l2' or 'cosine'"):
        MultiTableIndexer([_Hasher()], corpus, lambda a, b: 0)


def _bare(generation=0):
    """A MultiTableIndexer without tables: what the argument checks of a query need, nothing a device call could use."""
    from nlsh_amd.multitable import MultiTableIndexer
    ix = object.__new__(MultiTableIndexer)
    ix.tables, ix.generation = [], generation
    return ix


def test_query_refuses_k_and_foreign_or_stale_filters_before_touching_a_table():
    """`tables` is empty: a call that got past its argument checks would raise IndexError, not ValueError."""
    from nlsh_amd.indexer import RowFilter
    from nlsh_amd.multitable import MultiRowFilter
    ix, other = _bare(generation=3), _bare(generation=3)
    q = object()
    for call in (ix.query_tensors, ix.query):
        for k in (0, 257, 1000):
            with pytest.raises(ValueError, match=r"k in \[1, 256\]"):
                call(q, k=k)
        single = RowFilter(ix, None, 5, 3)
        with pytest.raises(ValueError, match="RowFilter of a single table"):
            call(q, filter=single)
        with pytest.raises(ValueError, match="must be None or a MultiRowFilter"):
            call(q, filter=[single])
        with pytest.raises(ValueError, match="built by another index"):
            call(q, filter=MultiRowFilter(other, [single], 3))
        with pytest.raises(ValueError, match="stale filter: built at generation 2, the index is at 3"):
            call(q, filter=MultiRowFilter(ix, [single], 2))
        with pytest.raises(IndexError):                       # the good filter passes the checks and reaches the (absent) tables
            call(q, filter=MultiRowFilter(ix, [single], 3))


def test_the_package_exports_the_facade_and_nothing_pipelined():
    import nlsh_amd
    from nlsh_amd import multitable
    assert nlsh_amd.MultiTableIndexer is multitable.MultiTableIndexer and nlsh_amd.MultiRowFilter is multitable.MultiRowFilter
    public = {n for n in dir(multitable.MultiTableIndexer) if not n.startswith("_")}
    assert {"query", "query_tensors", "add", "remove", "update", "row_filter"} <= public
    assert not {n for n in public if "pipeline" in n or "graph" in n or "shard" in n or "step" in n}
    doc = multitable.__doc__
    assert "no pipelined, graph-slot or sharded" in doc and 'storage="uint8"' in doc


# ----------------------------------------------------------------------------------------------- the reference against the definition
def _instance(rng, G, k):
    """G complete candidate sets of one query over a small id universe with few distance words: a row has ONE distance whichever list
    holds it (the precondition), lists overlap heavily, some are shorter than k, some empty."""
    n_ids = int(rng.integers(1, 4 * k + 3))
    dist = rng.choice(np.array([-1.5, 0.0, 0.25, 0.25, 3.0, np.inf], np.float32), size=n_ids)
    ids = rng.choice(np.arange(-5, 10 * n_ids), size=n_ids, replace=False)
    universe = M.T.make_keys(dist, ids)
    lists = []
    for _ in range(G):
        take = rng.random(n_ids) < rng.choice([0.0, 0.2, 0.6, 1.0])
        lists.append(universe[take])
    return lists


def test_unique_merge_of_per_list_topk_is_the_topk_of_the_union():
    """The fact the feature rests on: within a list the keys are distinct, so every member of the union's k best is among the k best
    of at least one list -- merging the G truncated lists and counting equal keys once loses nothing."""
    rng = np.random.default_rng(5)
    n_short = n_dup = 0
    for trial in range(400):
        G, k = int(rng.integers(1, 17)), int(rng.choice([1, 2, 5, 10, 33, 64, 100]))
        lists = _instance(rng, G, k)
        stride = k + int(rng.integers(0, 3))
        keys_in = M.per_list_topk(lists, k, stride)[:, None, :]                                  # [G, 1, stride]
        keys_in[:, :, k:] = rng.integers(1, 2 ** 62, size=(G, 1, stride - k), dtype=np.uint64)   # junk behind the lists is not read
        dist, idx, keys = M.unique_merge_reference(keys_in, k)
        want = M.union_topk(lists, k)
        assert np.array_equal(keys[0], want), trial
        wd, wi = M.split_keys(want)
        assert np.array_equal(dist.view(np.uint32)[0], wd.view(np.uint32)) and np.array_equal(idx[0], wi)
        real = want != M.KEY_NONE
        assert np.all(np.diff(want[real].astype(object)) > 0) and not real[int(real.sum()):].any()
        n_short += int(real.sum() < k)
        n_dup += int(sum(len(l) for l in lists) > len(np.unique(np.concatenate(lists + [np.zeros(0, np.uint64)]))))
    assert n_short > 20 and n_dup > 200                                                          # the instances are what they claim


def test_on_disjoint_lists_the_reference_is_the_plain_merge():
    rng = np.random.default_rng(6)
    for k in (1, 10, 65):
        G, Q = 5, 4
        pool = rng.permutation(np.arange(1, 20 * G * k * Q, dtype=np.uint64))[:G * Q * k].reshape(G, Q, k)
        keys_in = np.sort(pool, axis=2)
        keys_in[1, :, k // 2:] = M.KEY_NONE
        dist, idx, _ = M.unique_merge_reference(keys_in, k)
        pd, pi = M.T.merge_reference(keys_in, k)
        assert np.array_equal(dist.view(np.uint32), pd.view(np.uint32)) and np.array_equal(idx, pi)
