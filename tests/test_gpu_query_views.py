"""Strided and misaligned views as queries, encoder inputs and corpora.

The C ABI takes any q_stride >= d and any 4-byte-aligned pointer (include/nlsh_hip.h) and the facade forwards a view as it is (it copies
only when stride(1) != 1).  The layout then picks code paths at run time: the tiled scan reads the caller's queries directly with
16-byte scalar loads when the metric is exact L2, d % 4 == 0, q_stride % 4 == 0 and the base is 16-byte aligned, and a padded copy
otherwise (written by bplan_kernel, or by the encoder's epilogue for nlsh_query_batch and the batch slots); the fused encoder stages its
input with 16-byte or scalar loads by the same kind of test; gather_rows does the same for the corpus; a graph slot re-decides per
batch and pushes the decision into its captured graph.

A view is buf[:, o:o+d] of a device tensor buf[rows, W] whose other columns hold a finite sentinel:
    A   W = d + 4, o = 4    stride != d but everything aligned: the direct path with a stride
    B   W = d + 4, o = 2    stride % 4 == 0, base 8 mod 16: the copy is forced by the pointer clause alone
    C   W = d + 3, o = 1    odd stride, base 4 mod 16
    R   contig[5:]          a row slice
The data is the same in every layout; the contiguous tensor is the control, and the chain ends at the oracle."""
import numpy as np
import pytest
import torch

from helpers import dev, make_hashing
from nlsh_amd import _capi, synth
from oracle import oracle

pytestmark = pytest.mark.gpu

LAYOUTS = {"A": (4, 4, 0), "B": (4, 2, 8), "C": (3, 1, 4)}     # name -> (W - d, o, base address mod 16)
SENTINEL = 1000.0                                                # what the columns around a view hold: finite, and wrong everywhere


def as_view(x, name):
    """Device tensor of x's values in layout `name` ("contig" | "A" | "B" | "C"); x: numpy [rows, d] or a contiguous device tensor."""
    xd = x if torch.is_tensor(x) else dev(x)
    if name == "contig":
        return xd
    rows, d = xd.shape
    extra, o, mod16 = LAYOUTS[name]
    buf = torch.full((rows, d + extra), SENTINEL, dtype=torch.float32, device=xd.device)
    buf[:, o:o + d] = xd
    v = buf[:, o:o + d]
    assert v.stride() == (d + extra, 1) and v.data_ptr() % 16 == mod16 and not v.is_contiguous()
    return v


def _gen(metric):
    return synth.sift_like if metric == "l2" else synth.glove_like


def _dist_fn(metric):
    from nlsh_amd.data import Glove, SIFT
    return SIFT.distance if metric == "l2" else Glove.distance


# ------------------------------------------------------------------------------------ scan_tensors with given keys
@pytest.fixture(scope="module", params=[("l2", 128), ("l2", 25), ("cosine", 128), ("cosine", 25)], ids=lambda p: f"{p[0]}-{p[1]}")
def keyed(request):
    """~4 k rows in 30 buckets of ~135 rows (1- to 3-tile tasks), 70 queries x 4 probes, and the oracle's answer: once per (metric, d)."""
    metric, d = request.param
    rng = np.random.default_rng(17 * d + len(metric))
    N, Qn, P, k, nb = 4000, 70, 4, 10, 30
    corpus, queries = _gen(metric)(N, d, seed=500 + d), _gen(metric)(Qn, d, seed=501 + d)
    corpus[N // 2:N // 2 + 20] = corpus[:20]
    corpus_keys = (rng.integers(0, nb, N) * 3 - 40).astype(np.int32)
    tab = np.stack([rng.choice(nb, P, replace=False) * 3 - 40 for _ in range(Qn)]).astype(np.int32)
    tab[7, 1] = 777777                                               # an unknown key
    cnt = np.full(Qn, P, np.int32)
    cnt[9] = 2                                                       # fewer valid slots than columns
    perm, uniq, offs = oracle.build_csr(corpus_keys.astype(np.int64))
    ref = oracle.query_batch(corpus, perm, uniq, offs, queries, tab.astype(np.int64), cnt, k, metric)
    Ws, bs = synth.make_weights([d, 8, 16], seed=d)
    hashing = make_hashing(d, (8,), 16, Ws, bs, compat=False)       # not used: the keys are injected
    return dict(metric=metric, d=d, k=k, corpus=dev(corpus), queries=queries, keys=dev(corpus_keys), tab=dev(tab), cnt=dev(cnt), ref=ref,
                hashing=hashing)


@pytest.mark.parametrize("algo", ["query", "bucket", "tiled"])
def test_scan_of_query_views_equals_the_contiguous_scan(keyed, algo):
    from nlsh_amd.indexer import Indexer
    c = keyed
    ix = Indexer(c["hashing"], c["corpus"], _dist_fn(c["metric"]), compat=False, algo=algo, corpus_keys=c["keys"])
    contig = dev(c["queries"])
    d0, i0, n0, _ = ix.scan_tensors(contig, c["tab"], c["cnt"], k=c["k"])
    od, oi, onc = c["ref"]
    assert np.array_equal(n0.cpu().numpy(), onc)
    if algo == "tiled" and c["metric"] == "l2":                     # the control itself ends at the oracle, bit for bit
        assert np.array_equal(i0.cpu().numpy(), oi) and np.array_equal(d0.cpu().numpy().view(np.uint32), od.view(np.uint32))
    for name in LAYOUTS:
        d1, i1, n1, _ = ix.scan_tensors(as_view(contig, name), c["tab"], c["cnt"], k=c["k"])
        assert torch.equal(d1.view(torch.int32), d0.view(torch.int32)), name
        assert torch.equal(i1, i0) and torch.equal(n1, n0), name
    rows = contig[5:]                                                # R: rows 5.. of the same tensor (d = 25: base 4 mod 16)
    assert rows.data_ptr() == contig.data_ptr() + 5 * 4 * c["d"]
    d1, i1, n1, _ = ix.scan_tensors(rows, c["tab"][5:].contiguous(), c["cnt"][5:].contiguous(), k=c["k"])
    assert torch.equal(d1.view(torch.int32), d0[5:].view(torch.int32)) and torch.equal(i1, i0[5:]) and torch.equal(n1, n0[5:])


# ------------------------------------------------------------------------------------ the encoder on views
@pytest.mark.parametrize("n_rows", [130, 4100, 8300, 16500])     # the 16-row, 32-row, mixed and 128-row forms of the fused encoder
@pytest.mark.parametrize("d", [128, 25])
def test_encoder_on_views_is_the_oracle_bit_for_bit(d, n_rows):
    Ws, bs = synth.make_weights([d, 64, 64, 12], seed=d)
    hashing = make_hashing(d, (64, 64), 12, Ws, bs)
    x = synth.glove_like(n_rows, d, seed=600 + d)
    want_z = oracle.mlp_forward(x, Ws, bs).view(np.uint32)
    xd = dev(x)
    k0, c0 = hashing.hash_device(xd, n=4, seed=11)
    for name in ("contig",) + tuple(LAYOUTS):
        v = as_view(xd, name)
        z, _, _ = hashing.forward_device(v)
        assert np.array_equal(z.cpu().numpy().view(np.uint32), want_z), name
        k1, c1 = hashing.hash_device(v, n=4, seed=11)
        assert torch.equal(k1, k0) and torch.equal(c1, c0), name


# ------------------------------------------------------------------------------------ one nlsh_query_batch call
@pytest.fixture(scope="module", params=[("l2", 128), ("l2", 25), ("cosine", 128), ("cosine", 25)], ids=lambda p: f"{p[0]}-{p[1]}")
def hashed(request):
    metric, d = request.param
    Ws, bs = synth.make_weights([d, 64, 64, 8], seed=20 + d)
    return dict(metric=metric, d=d, hashing=make_hashing(d, (64, 64), 8, Ws, bs), corpus=dev(_gen(metric)(20000, d, seed=700 + d)))


@pytest.mark.parametrize("algo", ["bucket", "tiled"])
def test_one_call_batch_on_query_views_equals_the_contiguous_call(hashed, algo):
    from nlsh_amd.indexer import Indexer
    c = hashed
    ix = Indexer(c["hashing"], c["corpus"], _dist_fn(c["metric"]), algo=algo)
    for Qn in (130, 4100):
        contig = dev(_gen(c["metric"])(Qn, c["d"], seed=800 + Qn))
        want = ix._batch_tensors(contig, 10, 3, 4242)
        assert ix._fuses(contig, 3, ix.last_algo)                    # it was the one-call form
        assert int(want[2].max()) > 0
        for name in LAYOUTS:
            got = ix._batch_tensors(as_view(contig, name), 10, 3, 4242)
            assert torch.equal(got[4], want[4]) and torch.equal(got[5], want[5]), (Qn, name)              # key table, nkeys
            assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (Qn, name)           # distance bits
            assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), (Qn, name)              # ids, candidate counts


# ------------------------------------------------------------------------------------ graph slots and staged slots
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "staged"])
def test_batch_slots_take_a_different_layout_every_batch(graph):
    """Exact L2 at d = 128: contiguous and A take the direct query path, B and C the copied one.  Two slots as the sequence is given;
    with three slots every slot's consecutive batches are on different sides of that decision (contiguous -> B, C -> contiguous, A -> C),
    which a graph slot has to push into its captured graph (hipGraphExecKernelNodeSetParams)."""
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.pipeline import QueryPipeline
    d, N, Qn, H, k, P = 128, 20000, 256, 8, 10, 4
    corpus = synth.sift_like(N, d, seed=41)
    Ws, bs = synth.make_weights([d, 64, H], seed=41)
    ix = Indexer(make_hashing(d, (64,), H, Ws, bs, compat=False), dev(corpus), SIFT.distance, compat=False, algo="tiled")
    layouts = ["contig", "C", "A", "B", "contig", "C"]
    batches = [as_view(synth.sift_like(Qn, d, seed=50 + i), name) for i, name in enumerate(layouts)]
    want = []
    for i, b in enumerate(batches):
        w = [t.clone() for t in ix.query_tensors(b, k=k, hash_times=P, seed=900 + i, want_keys=True)]
        for a, t in zip(ix.query_tensors(b.contiguous(), k=k, hash_times=P, seed=900 + i, want_keys=True), w):
            assert torch.equal(a, t), (i, layouts[i])
        want.append(w)
    for depth in (2, 3):
        pipe = QueryPipeline(ix, batches[0], k=k, hash_times=P, depth=depth, want_keys=True, graph=graph)
        assert pipe.graph == graph
        got = []
        for i, b in enumerate(batches):
            got.append(pipe.submit(b, seed=900 + i))
            if (i + 1) % depth == 0 or i + 1 == len(batches):       # a slot is overwritten `depth` submits later: read now
                pipe.synchronize()
                for j in range(i + 1 - ((i % depth) + 1), i + 1):
                    for a, w in zip(got[j], want[j]):
                        assert torch.equal(a, w), (depth, j, layouts[j])
        assert not pipe.overflowed()
        pipe.close()


# ------------------------------------------------------------------------------------ an index built from a corpus view
@pytest.mark.parametrize("d", [128, 25])
def test_index_built_from_a_corpus_view_equals_the_contiguous_build(d):
    from nlsh_amd.data import Glove
    from nlsh_amd.indexer import Indexer
    Ws, bs = synth.make_weights([d, 64, 10], seed=d)
    hashing = make_hashing(d, (64,), 10, Ws, bs)
    corpus = dev(synth.glove_like(5000, d, seed=900 + d))
    base = Indexer(hashing, corpus, Glove.distance)
    assert base.n_buckets > 1
    for name in ("B", "C"):
        ix = Indexer(hashing, as_view(corpus, name), Glove.distance)
        for what in ("corpus_sorted", "inv_norm", "gid", "uniq_keys", "offsets"):
            a, b = getattr(ix, what), getattr(base, what)
            assert a.dtype == b.dtype and a.shape == b.shape, (name, what)
            assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), (name, what)
