"""Categorical hashing on the GPU: `nlsh_encode_logits` against the oracle's MLP bit for bit, `nlsh_probe_bins` / `_budget` against the numpy
reference of tests/categorical_ref.py in every word, and `Indexer(Categorical)` end to end against the same index built from the reference's
argmax keys and scanned on the reference's key table.  Nothing has a tolerance."""
import functools

import numpy as np
import pytest
import torch

import categorical_ref as cr
from helpers import dev

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------- shared, computed once
def weights(dims, bias, seed):
    """Seeded nn.Linear-layout weights of a layer stack; `bias` False: bias-free hidden layers (the output layer keeps its bias)."""
    rng = np.random.default_rng(seed)
    Ws = [(rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32) for l in range(len(dims) - 1)]
    bs = [(0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32) if bias or l + 2 == len(dims) else None for l in range(len(dims) - 1)]
    return Ws, bs


def make_categorical(dims, Ws, bs):
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.hashings import Categorical

    class Identity(torch.nn.Module):      # a single Linear layer: the hash is the output layer on the input itself
        output_dim = dims[0]

        def forward(self, x):
            return x

        def linear_stack(self):
            return []
    enc = MultiLayerRelu(dims[0], list(dims[1:-1]), with_bias=bs[0] is not None) if len(dims) > 2 else Identity()
    h = Categorical(enc, dims[-1], None)
    lin = [m for m in h._hasher.modules() if isinstance(m, torch.nn.Linear)]
    assert len(lin) == len(Ws)
    with torch.no_grad():
        for m, W, b in zip(lin, Ws, bs):
            m.weight.copy_(torch.from_numpy(W))
            if b is not None:
                m.bias.copy_(torch.from_numpy(b))
    h.train_mode(False)
    return h


ROWS_MAX = 4097
LOGIT_DIMS = ([128, 256], [128, 256, 256], [25, 633, 100], [100, 64, 4096], [96, 1024, 1000], [1024, 512, 1])


@functools.lru_cache(maxsize=None)
def logits_case(dims, bias):
    """(x [4097, d], weights, the oracle's logits) of one layer stack; the 1 / 130 / 4097-row tests read prefixes of it."""
    from oracle import oracle
    dims = list(dims)
    Ws, bs = weights(dims, bias, seed=sum(dims) + bias)
    x = np.random.default_rng(len(dims) + dims[0]).standard_normal((ROWS_MAX, dims[0])).astype(np.float32)
    return x, Ws, bs, oracle.mlp_forward(x, Ws, bs)


def bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


# ---------------------------------------------------------------------------- the logits forward
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("dims", LOGIT_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_logits_are_the_oracles_bits(dims, bias):
    x, Ws, bs, want = logits_case(tuple(dims), bias)
    h = make_categorical(dims, Ws, bs)
    xd = dev(x)
    for rows in (1, 130, ROWS_MAX):
        got = h.logits_device(xd[:rows])
        assert got.shape == (rows, dims[-1]) and np.array_equal(bits(got), bits(want[:rows])), (dims, bias, rows)
    p = h.predict(xd[:130])                                            # eval mode: torch.softmax of those logits
    assert torch.equal(p, torch.softmax(h.logits_device(xd[:130]), dim=1))


@pytest.mark.parametrize("dims", [[25, 633, 100], [128, 256, 256]], ids=lambda d: "x".join(map(str, d)))
def test_logits_of_a_strided_misaligned_view_two_workspace_sizes_and_a_wide_output_row(dims):
    """The C call itself: x rows at an odd stride from an address 4 bytes off a 16-byte boundary, a workspace of one 128-row tile against
    one for every row (33 passes against 1), and an output stride above M whose columns >= M keep their sentinel."""
    from nlsh_amd import _capi
    x, Ws, bs, want = logits_case(tuple(dims), True)
    h = make_categorical(dims, Ws, bs)
    L, n, d, M = _capi.lib(), ROWS_MAX, dims[0], dims[-1]
    stride = d + 3
    flat = torch.zeros(n * stride + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(n, stride)[:, :d]
    view.copy_(dev(x))
    assert view.data_ptr() % 16 == 4 and view.stride(0) == stride
    packed, arr = h.packed_weights(), _capi.int_array(dims)
    outs = []
    for rows_per_pass in (1, n):
        ws = torch.empty(L.nlsh_logits_workspace(rows_per_pass, len(dims) - 1, arr), dtype=torch.uint8, device="cuda")
        out = torch.full((n, M + 5), -7.0, dtype=torch.float32, device="cuda")
        _capi.check(L.nlsh_encode_logits(_capi.ptr(view), n, stride, len(dims) - 1, arr, _capi.ptr(packed), _capi.ptr(out), M + 5,
                                         _capi.ptr(ws), ws.numel(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert bool((out[:, M:] == -7.0).all()), "a column >= M was written"
        outs.append(out[:, :M].contiguous())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert np.array_equal(bits(outs[0]), bits(want))
    small = torch.empty(1024, dtype=torch.uint8, device="cuda")
    rc = L.nlsh_encode_logits(_capi.ptr(view), n, stride, len(dims) - 1, arr, _capi.ptr(packed), _capi.ptr(outs[0]), M, _capi.ptr(small), 1024, None)
    assert rc == _capi.E_WORKSPACE


# ---------------------------------------------------------------------------- nlsh_probe_bins
def probe(logits, M, P, n_multi_rows=None, uniq=None, offsets=None, budget=None):
    """One `nlsh_probe_bins` (budget None) or `nlsh_probe_bins_budget` call on a device tensor or view -> numpy (keys, nkeys, logit bits[,
    ncand]); every output starts as a sentinel."""
    from nlsh_amd import _capi
    n = logits.shape[0]
    keys = torch.full((n, P), -7, dtype=torch.int32, device="cuda")
    nkeys = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    lg = torch.full((n, P), -7.0, dtype=torch.float32, device="cuda")
    head = (_capi.ptr(logits), logits.stride(0), n, M, P, n if n_multi_rows is None else n_multi_rows)
    stream = torch.cuda.current_stream().cuda_stream
    if budget is None:
        _capi.check(_capi.lib().nlsh_probe_bins(*head, _capi.ptr(keys), _capi.ptr(nkeys), _capi.ptr(lg), stream))
        torch.cuda.synchronize()
        return keys.cpu().numpy(), nkeys.cpu().numpy(), bits(lg)
    ncand = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    _capi.check(_capi.lib().nlsh_probe_bins_budget(*head, _capi.ptr(uniq), _capi.ptr(offsets), 0 if uniq is None else uniq.shape[0], budget,
                                                   _capi.ptr(keys), _capi.ptr(nkeys), _capi.ptr(lg), _capi.ptr(ncand), stream))
    torch.cuda.synchronize()
    return keys.cpu().numpy(), nkeys.cpu().numpy(), bits(lg), ncand.cpu().numpy()


def assert_table(got, want, what):
    for name, g, w in zip(("keys", "nkeys", "logit bits", "ncand"), got, want):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())


M_ALL = (1, 2, 63, 64, 65, 100, 256, 1000, 4096)
P_ALL = (1, 2, 10, 64, 128)


@functools.lru_cache(maxsize=None)
def rows_case(M):
    """257 rows of M logits: random, mass ties, +-inf / signed zeros and all-equal rows, interleaved."""
    return cr.mixed_rows(257, M, seed=3 * M + 1)


@pytest.mark.parametrize("M", M_ALL)
def test_probe_bins_equals_the_reference_in_every_word(M):
    z = rows_case(M)
    zd = dev(z)
    for P in P_ALL:
        want = cr.table(z, P)
        for rows in (1, 3, 257):
            assert_table(probe(zd[:rows], M, P), [w[:rows] for w in want], (M, P, rows))
        assert_table(probe(zd, M, P, n_multi_rows=130), cr.table(z, P, n_multi_rows=130), (M, P, "n_multi_rows"))


@pytest.mark.parametrize("M", [65, 100, 1000])
def test_probe_bins_on_strided_views(M):
    """A row stride above M: a 16-byte-aligned one (vector loads) and an odd one from a misaligned base (scalar loads)."""
    z = rows_case(M)
    for pad, shift in ((M % 4 and 4 - M % 4 or 4, 0), (3, 1)):
        stride = M + pad
        flat = torch.full((257 * stride + shift,), 9.0e37, dtype=torch.float32, device="cuda")      # larger than every finite logit but one
        view = flat[shift:].view(257, stride)[:, :M]
        view.copy_(dev(z))
        for P in (10, 128):
            assert_table(probe(view, M, P), cr.table(z, P), (M, P, stride, shift))


def test_probe_bins_equal_rows_signed_zeros_and_infinities():
    for M in (1, 64, 100, 4096):
        for P in (1, 10, 128):
            keys, nkeys, lg = probe(dev(cr.equal_rows(5, M)), M, P)
            n = min(P, M)
            assert (keys[:, :n] == np.arange(n)[None, :]).all() and not keys[:, n:].any() and nkeys.tolist() == [n] * 5
            assert (lg[:, :n] == np.float32(0.75).view(np.uint32)).all() and (lg[:, n:] == cr.NEG_INF_BITS).all()
    z = np.array([[-0.0, 0.0, -0.0, 0.0, -np.inf, np.inf, 1.0, -1.0]], dtype=np.float32).repeat(4, 0)
    keys, nkeys, lg = probe(dev(z), 8, 10)
    assert keys[:, :8].tolist() == [[5, 6, 1, 3, 0, 2, 7, 4]] * 4 and nkeys.tolist() == [8] * 4
    assert np.array_equal(lg[:, :8], z[:, [5, 6, 1, 3, 0, 2, 7, 4]].view(np.uint32))
    for M in (65, 1000):
        z = cr.special_rows(40, M, seed=M)
        for P in (2, 64, 128):
            assert_table(probe(dev(z), M, P), cr.table(z, P), ("special", M, P))


# ---------------------------------------------------------------------------- the budget form
@functools.lru_cache(maxsize=None)
def built_csr(M):
    """A REAL CSR (`nlsh_build_csr` through an Indexer-free call): one key per corpus row drawn from 60 % of the bins with a skewed
    law, so probed bins have buckets of very different sizes or none."""
    from nlsh_amd import _capi
    rng = np.random.default_rng(M)
    live = np.nonzero(rng.random(M) < 0.6)[0][:M - 1]                  # at least one bin has no bucket
    if len(live) == 0:
        live = np.array([0])
    w = rng.random(len(live)) ** 4
    keys = rng.choice(live, size=5000, p=w / w.sum()).astype(np.int32)
    L, kd = _capi.lib(), dev(keys)
    n = len(keys)
    perm, uniq, offsets = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
                           torch.empty(n + 1, dtype=torch.int32, device="cuda"))
    nb = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.nlsh_build_csr_workspace(n), dtype=torch.uint8, device="cuda")
    _capi.check(L.nlsh_build_csr(_capi.ptr(kd), n, _capi.ptr(perm), _capi.ptr(uniq), _capi.ptr(offsets), _capi.ptr(nb), _capi.ptr(ws),
                                 ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    b = int(nb.item())
    uniq, offsets = uniq[:b].contiguous(), offsets[:b + 1].contiguous()
    want_u, want_c = np.unique(keys, return_counts=True)
    assert np.array_equal(uniq.cpu().numpy(), want_u) and np.array_equal(np.diff(offsets.cpu().numpy()), want_c)
    return uniq, offsets


@pytest.mark.parametrize("M", [2, 64, 100, 1000, 4096])
def test_probe_bins_budget_equals_the_reference_on_a_built_csr(M):
    z = rows_case(M)
    zd = dev(z)
    uniq, offsets = built_csr(M)
    un, on = uniq.cpu().numpy(), offsets.cpu().numpy()
    stopped = missing = 0
    for P in (1, 10, 128):
        full = cr.table(z, P, n_multi_rows=200)
        unb = cr.cut(*full, un, on, cr.INT32_MAX)
        mid = max(1, int(np.median(unb[3]) // 2))
        for budget in (1, mid, cr.INT32_MAX):
            want = cr.cut(*full, un, on, budget)
            assert_table(probe(zd, M, P, 200, uniq, offsets, budget), want, (M, P, budget))
            stopped += int((want[1] < full[1]).sum())
        assert_table(probe(zd, M, P, 200, uniq, offsets, cr.INT32_MAX)[:3], probe(zd, M, P, 200), (M, P, "INT32_MAX is the unbudgeted call"))
        valid = np.arange(P)[None, :] < full[1][:, None]
        missing += int((~np.isin(full[0], un) & valid).sum())
        none = probe(zd, M, P, 200, None, None, 1)                         # n_buckets = 0: no row stops early, every count is 0
        assert_table(none[:3], full, (M, P, "empty index"))
        assert not none[3].any()
    assert stopped and missing                                         # rows do stop early, and probed bins without a bucket occur


# ---------------------------------------------------------------------------- end to end
N_CORPUS, N_QUERIES, DIM = 3000, 200, 32


@functools.lru_cache(maxsize=None)
def world(M):
    """Corpus, queries, a Categorical hasher of M bins with seeded weights, the reference's keys (the oracle's logits through the numpy
    definition) and the two indexes: built by the hasher, and built from the reference's argmax keys."""
    from nlsh_amd import synth
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    from oracle import oracle
    corpus, mean, std = synth.standardise(synth.sift_like(N_CORPUS, DIM))
    queries, _, _ = synth.standardise(synth.sift_like(N_QUERIES, DIM, seed=synth.SEED_QUERY), mean, std)
    dims = [DIM, 64, M]
    Ws, bs = weights(dims, True, seed=M)
    h = make_categorical(dims, Ws, bs)
    corpus_logits, query_logits = oracle.mlp_forward(corpus, Ws, bs), oracle.mlp_forward(queries, Ws, bs)
    corpus_keys = cr.table(corpus_logits, 1)[0][:, 0].copy()
    cd, qd = dev(corpus), dev(queries)
    ix = Indexer(h, cd, SIFT.distance, compat=False)
    ref = Indexer(h, cd, SIFT.distance, compat=False, corpus_keys=dev(corpus_keys))
    return dict(corpus=corpus, queries=queries, cd=cd, qd=qd, h=h, corpus_keys=corpus_keys, query_logits=query_logits, ix=ix, ref=ref,
                distance=SIFT.distance)


def query_table(w, P):
    keys, nkeys, _ = cr.table(w["query_logits"], P)
    return keys, nkeys


def same_result(a, b, what):
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), what


@pytest.mark.parametrize("M", [16, 100])
def test_the_index_is_the_one_built_from_the_reference_argmax(M):
    w = world(M)
    ix, ref, h = w["ix"], w["ref"], w["h"]
    assert np.array_equal(ix.corpus_keys.cpu().numpy(), w["corpus_keys"])
    for name in ("gid", "uniq_keys", "offsets", "corpus_keys"):
        assert torch.equal(getattr(ix, name), getattr(ref, name)), name
    assert ix.n_buckets == ref.n_buckets == len(np.unique(w["corpus_keys"])) <= M
    assert h.hash(w["qd"][:50]) == cr.table(w["query_logits"][:50], 1)[0][:, 0].tolist()          # n=None: the reference's List[int]
    keys, nkeys = query_table(w, 5)
    assert h.hash(w["qd"][:50], n=5) == [set(keys[r, :nkeys[r]].tolist()) for r in range(50)]
    assert set(ix.index2row) == set(np.unique(w["corpus_keys"]).tolist())


@pytest.mark.parametrize("hash_times", [1, 10, 100])
@pytest.mark.parametrize("M", [16, 100])
def test_queries_equal_the_scan_on_the_reference_key_table_and_the_oracle(M, hash_times):
    from oracle import oracle
    w = world(M)
    ix, ref, qd = w["ix"], w["ref"], w["qd"]
    keys, nkeys = query_table(w, hash_times)
    hk, hn = ix.hash_device(qd, hash_times=hash_times)
    assert np.array_equal(hk.cpu().numpy(), keys) and np.array_equal(hn.cpu().numpy(), nkeys)
    ox = oracle.OracleIndexer.from_keys(w["corpus"], w["corpus_keys"], key_mode="full")
    key_lists = [keys[r, :nkeys[r]].tolist() for r in range(N_QUERIES)]
    for k in (1, 10, 100):
        got = ix.query_tensors(qd, k=k, hash_times=hash_times)
        assert ix.last_query_path == "two_step"
        same_result(got, ref.scan_tensors(qd, dev(keys), dev(nkeys), k=k), (M, hash_times, k))
        ids, counts = ix.query(qd, k=k, hash_times=hash_times)
        assert ix.last_query_path == "two_step"
        olists, ocounts, _, oidx = ox.query_with_keys(w["queries"], key_lists, k=k)
        assert counts == ocounts == got[2].cpu().tolist()
        for r in range(N_QUERIES):                                     # compat=False: min(k, candidates) ids, no last-key rule
            assert ids[r] == (olists[r] if ocounts[r] >= k else [int(v) for v in oidx[r] if v >= 0]), (M, hash_times, k, r)


def test_compat_keeps_the_trailing_partial_batch_single_probe():
    w = world(16)
    from nlsh_amd.indexer import Indexer
    ix = Indexer(w["h"], w["cd"], w["distance"], corpus_keys=dev(w["corpus_keys"]))          # compat=True
    hk, hn = ix.hash_device(w["qd"], batch_size=64, hash_times=4)
    keys, nkeys, _ = cr.table(w["query_logits"], 4, n_multi_rows=192)
    assert np.array_equal(hk.cpu().numpy(), keys) and np.array_equal(hn.cpu().numpy(), nkeys) and nkeys[192:].tolist() == [1] * 8


@pytest.mark.parametrize("M", [16, 100])
def test_candidate_budget(M):
    w = world(M)
    ix, ref, qd = w["ix"], w["ref"], w["qd"]
    P = 20
    full = cr.table(w["query_logits"], P)
    un, on = ix.uniq_keys.cpu().numpy(), ix.offsets.cpu().numpy()
    stopped = 0
    for budget in (1, 150, 10 ** 12):
        want = cr.cut(*full, un, on, min(budget, cr.INT32_MAX))
        hk, hn = ix.hash_device(qd, hash_times=P, candidate_budget=budget)
        assert np.array_equal(hk.cpu().numpy(), want[0]) and np.array_equal(hn.cpu().numpy(), want[1])
        got = ix.query_tensors(qd, k=10, hash_times=P, candidate_budget=budget)
        assert ix.last_query_path == "two_step" and np.array_equal(got[2].cpu().numpy(), want[3])
        same_result(got, ref.scan_tensors(qd, dev(want[0]), dev(want[1]), k=10), (M, budget))
        ids, counts = ix.query(qd, k=10, hash_times=P, candidate_budget=budget)
        assert counts == want[3].tolist() and ids == ref.query_with_keys(qd, [want[0][r, :want[1][r]].tolist() for r in range(N_QUERIES)], k=10)[0]
        stopped += int((want[1] < full[1]).sum())
    assert stopped


def _pair(w, **kw):
    """(index built by the hasher, index built from the reference keys) with the same extra constructor arguments."""
    from nlsh_amd.indexer import Indexer
    return (Indexer(w["h"], w["cd"], w["distance"], compat=False, **kw),
            Indexer(w["h"], w["cd"], w["distance"], compat=False, corpus_keys=dev(w["corpus_keys"]), **kw))


def _sq8_pair(w, **kw):
    """`_pair` for storage="sq8".  A compressed index hashes the rows as it holds them, so the reference keys are the argmax of the oracle's
    logits on the DEQUANTISED rows, and the second index takes the first one's quantiser: both hold the same codes."""
    from nlsh_amd.indexer import Indexer
    from oracle import oracle
    ix = Indexer(w["h"], w["cd"], w["distance"], compat=False, storage="sq8", **kw)
    held = ix._dequantised(w["cd"]).cpu().numpy()
    lin = [m for m in w["h"]._hasher.modules() if isinstance(m, torch.nn.Linear)]
    Ws, bs = [m.weight.detach().cpu().numpy() for m in lin], [m.bias.detach().cpu().numpy() for m in lin]
    held_keys = cr.table(oracle.mlp_forward(held, Ws, bs), 1)[0][:, 0].copy()
    assert (held_keys != w["corpus_keys"]).any()                      # rounding the rows does move some of them to another bin
    ref = Indexer(w["h"], w["cd"], w["distance"], compat=False, storage="sq8", quantiser=ix.quantiser, corpus_keys=dev(held_keys), **kw)
    return ix, ref


def test_sq8_storage():
    w = world(100)
    ix, ref = _sq8_pair(w)
    keys, nkeys = query_table(w, 10)
    for name in ("gid", "uniq_keys", "offsets", "corpus_keys"):
        assert torch.equal(getattr(ix, name), getattr(ref, name)), name
    same_result(ix.query_tensors(w["qd"], k=10, hash_times=10), ref.scan_tensors(w["qd"], dev(keys), dev(nkeys), k=10), "sq8")


def test_refine_on_the_device():
    w = world(100)
    ix, ref = _pair(w, refine="device")
    keys, nkeys = query_table(w, 10)
    same_result(ix.query_tensors(w["qd"], k=10, hash_times=10), ref.scan_tensors(w["qd"], dev(keys), dev(nkeys), k=10), "refine")
    assert ix.last_query_path == "two_step+refine"
    assert ix.query(w["qd"], k=10, hash_times=10) == ref.query_with_keys(w["qd"], [keys[r, :nkeys[r]].tolist() for r in range(N_QUERIES)], k=10)[:2]


def test_row_filter():
    w = world(100)
    ix, ref = w["ix"], w["ref"]
    keys, nkeys = query_table(w, 10)
    allow = torch.arange(0, N_CORPUS, 3, dtype=torch.int32, device="cuda")
    got = ix.query_tensors(w["qd"], k=10, hash_times=10, filter=ix.row_filter(allow=allow))
    same_result(got, ref.scan_tensors(w["qd"], dev(keys), dev(nkeys), k=10, filter=ref.row_filter(allow=allow)), "filter")
    assert bool(((got[1] % 3 == 0) | (got[1] < 0)).all()) and ix.last_query_path == "two_step"


def test_tag_mask():
    w = world(100)
    tags = dev((1 << (np.arange(N_CORPUS) % 5)).astype(np.int64))
    ix, ref = _pair(w, tags=tags)
    keys, nkeys = query_table(w, 10)
    got = ix.query_tensors(w["qd"], k=10, hash_times=10, tag_mask=0b00110)
    same_result(got, ref.scan_tensors(w["qd"], dev(keys), dev(nkeys), k=10, tag_mask=0b00110), "tags")
    ok = got[1] >= 0
    assert bool(((got[1][ok] % 5 == 1) | (got[1][ok] % 5 == 2)).all()) and bool(ok.any())


def test_range_query():
    w = world(100)
    ix, ref = w["ix"], w["ref"]
    keys, nkeys = query_table(w, 10)
    radius = float(np.median(ix.query_tensors(w["qd"], k=10, hash_times=10)[0][:, 4].cpu().numpy()))
    got = ix.range_query(w["qd"], radius, hash_times=10)
    want = ref.range_query_with_keys(w["qd"], [keys[r, :nkeys[r]].tolist() for r in range(N_QUERIES)], radius)
    assert got == want and sum(map(len, got[0])) > 0 and ix.last_query_path == "two_step"


def test_add_and_remove_equal_the_rebuild():
    from nlsh_amd.indexer import Indexer
    w = world(100)
    h, cd = w["h"], w["cd"]
    ix = Indexer(h, cd[:2500], w["distance"], compat=False)
    ids = ix.add(cd[2500:])                                            # keys default to the hasher's: the Categorical argmax
    assert ids.cpu().tolist() == list(range(2500, N_CORPUS))
    for name in ("gid", "uniq_keys", "offsets", "corpus_keys"):
        assert torch.equal(getattr(ix, name), getattr(w["ix"], name)), name
    gone = torch.arange(0, N_CORPUS, 7, dtype=torch.int32, device="cuda")
    assert ix.remove(gone) == len(gone)
    keep = np.setdiff1d(np.arange(N_CORPUS), gone.cpu().numpy())
    rebuilt = Indexer(h, cd[dev(keep)], w["distance"], compat=False, row_ids=dev(keep.astype(np.int32)))
    same_result(ix.query_tensors(w["qd"], k=10, hash_times=10), rebuilt.query_tensors(w["qd"], k=10, hash_times=10), "add / remove")


def test_a_two_table_index():
    from nlsh_amd.multitable import MultiTableIndexer
    w, w2 = world(100), world(16)
    mt = MultiTableIndexer([w["h"], w2["h"]], w["cd"], w["distance"])
    want = MultiTableIndexer([w["h"], w2["h"]], w["cd"], w["distance"], corpus_keys=[dev(w["corpus_keys"]), dev(w2["corpus_keys"])])
    for a, b in zip(mt.tables, want.tables):
        assert torch.equal(a.gid, b.gid) and torch.equal(a.offsets, b.offsets)
    got = mt.query_tensors(w["qd"], k=10, hash_times=4)
    # the merge of the two tables' own results: every id is a candidate of one of them, counts add up
    one, two = w["ix"].query_tensors(w["qd"], k=10, hash_times=4), w2["ix"].query_tensors(w["qd"], k=10, hash_times=4)
    assert torch.equal(got[2], one[2] + two[2])
    both = torch.cat([one[0], two[0]], dim=1)
    assert torch.equal(got[0][:, 0], both.min(dim=1).values)
    same_result(got, want.query_tensors(w["qd"], k=10, hash_times=4), "two tables")


def test_pipelines_and_sharded_indexes_refuse_it():
    from nlsh_amd import _capi
    from nlsh_amd.distributed import ShardedIndexer
    from nlsh_amd.pipeline import QueryPipeline
    w = world(16)
    for graph in (True, False):
        with pytest.raises(_capi.NlshHipError, match="Categorical"):
            QueryPipeline(w["ix"], w["qd"], k=10, hash_times=4, graph=graph)
    with pytest.raises(NotImplementedError, match="Categorical"):
        ShardedIndexer(w["h"], w["cd"], w["distance"], id_base=0)
    with pytest.raises(ValueError, match="Bernoulli"):
        w["ix"].query_tensors(w["qd"], k=10, hash_times=4, probes="sampled")
    assert w["h"].probes == "ranked"


def test_kmeans_partition_and_fit_partition_give_a_usable_hash():
    """The trainer's device half: k-means labels are nearest-centroid assignments, and a hash fitted to them for a few steps puts most
    rows into their own bin."""
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.hashings import Categorical
    from nlsh_amd.training import fit_partition, kmeans_partition
    w = world(16)
    x = w["cd"][:1000]
    labels = kmeans_partition(x, 8, iters=5, seed=1)
    assert labels.shape == (1000,) and labels.dtype == torch.int64 and 0 <= int(labels.min()) and int(labels.max()) < 8
    assert torch.equal(labels, kmeans_partition(x, 8, iters=5, seed=1))
    centroids = torch.stack([x[labels == b].mean(0) for b in range(8) if bool((labels == b).any())])
    moved = (torch.cdist(x, centroids).argmin(1) != torch.unique(labels, return_inverse=True)[1]).float().mean()
    assert float(moved) < 0.1                                          # five Lloyd steps: close to a fixed point
    h = Categorical(MultiLayerRelu(DIM, [64]), 8, None)
    losses = fit_partition(h, x, labels, n_steps=200, batch_size=250, learning_rate=3e-3)
    assert np.mean(losses[-5:]) < 0.5 * np.mean(losses[:5])
    assert float((h.hash_device(x)[0][:, 0].long() == labels).float().mean()) > 0.8
