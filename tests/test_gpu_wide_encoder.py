"""GPU: encoders with hidden layers wider than the LDS-resident forms take (> 632), through the streamed form
(nlsh_encode_hash_stream): z bit-exact against the oracle's k-ordered fmaf chains, the epilogue's probabilities, codes and
multi-probe keys against the oracle, streamed == fused on narrow encoders, outputs independent of the workspace size, an index
built and queried end to end, a checkpoint round trip, and the pipelined batch slots' refusal."""

import numpy as np
import pytest
import torch

from helpers import dev, make_hashing
from nlsh_amd import _capi, synth
from oracle import oracle

pytestmark = pytest.mark.gpu

WIDE = [128, 1024, 1024, 16]


def _weights(dims, seed, hidden_bias=True):
    Ws, bs = synth.make_weights(dims, seed=seed)
    if not hidden_bias:
        bs = [None] * (len(dims) - 2) + [bs[-1]]     # bias-free encoder layers, the output layer keeps its bias (encoders.py:10,31)
    return Ws, bs


def _hashing(dims, Ws, bs, **kw):
    return make_hashing(dims[0], dims[1:-1], dims[-1], Ws, bs, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ----------------------------------------------------------------------------- 1. z bit-exact
@pytest.mark.parametrize("hidden_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dims", [WIDE, [25, 633, 8], [100, 2048, 24], [960, 4096, 512, 32], [1024, 1000, 1000, 1000, 7],
                                  [96, 640, 700, 640, 20]], ids=lambda d: "x".join(map(str, d)))
def test_wide_z_bit_exact_against_oracle(dims, hidden_bias):
    Ws, bs = _weights(dims, 17, hidden_bias)
    x = synth.glove_like(130, dims[0], seed=23)
    h = _hashing(dims, Ws, bs)
    assert h.streamed()
    z, _, _ = h.forward_device(dev(x))
    zo = oracle.mlp_forward(x, Ws, bs)
    assert np.array_equal(_bits(z.cpu().numpy()), _bits(zo)), f"max |dz| {np.abs(z.cpu().numpy() - zo).max()}"


@pytest.mark.parametrize("hidden_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("n_rows", [1, 31, 33, 4097])
def test_wide_z_bit_exact_at_ragged_row_counts(n_rows, hidden_bias):
    Ws, bs = _weights(WIDE, 5, hidden_bias)
    x, _, _ = synth.standardise(synth.sift_like(max(n_rows, 8), WIDE[0], seed=21))
    x = x[:n_rows]
    z, _, _ = _hashing(WIDE, Ws, bs).forward_device(dev(x))
    assert np.array_equal(_bits(z.cpu().numpy()), _bits(oracle.mlp_forward(x, Ws, bs)))


def test_wide_rows_with_a_stride_and_an_odd_input_width():
    """Layer 0 reads x as it is: a row stride wider than d (a column slice) and d % 4 != 0 take the scalar staging path."""
    dims = [25, 700, 8]
    Ws, bs = _weights(dims, 3)
    x = synth.glove_like(300, 27, seed=4)
    xd = dev(x)[:, 1:26]                       # stride 27, offset one float: neither 16-byte aligned nor a multiple of 4
    z, _, _ = _hashing(dims, Ws, bs).forward_device(xd)
    assert np.array_equal(_bits(z.cpu().numpy()), _bits(oracle.mlp_forward(x[:, 1:26], Ws, bs)))


# ----------------------------------------------------------------------------- 2. probs and code
@pytest.mark.parametrize("tanh", [False, True], ids=["sigmoid", "tanh"])
def test_wide_probs_and_code(tanh):
    Ws, bs = _weights(WIDE, 8)
    x, _, _ = synth.standardise(synth.sift_like(700, WIDE[0], seed=8))
    z, probs, code = _hashing(WIDE, Ws, bs, tanh=tanh).forward_device(dev(x))
    zh = z.cpu().numpy()
    raw_o, p01_o = oracle.head_probs(zh, "tanh" if tanh else "sigmoid")
    assert np.abs(probs.cpu().numpy() - raw_o).max() <= 2e-7
    p01 = probs.cpu().numpy() / 2 + 0.5 if tanh else probs.cpu().numpy()
    code_o = oracle.pack_keys(oracle.hard_bits(p01.astype(np.float32))[:, None, :], "full")[:, 0]
    assert np.array_equal(code.cpu().numpy().view(np.uint32).astype(np.int64), code_o)


# ----------------------------------------------------------------------------- 3. multi-probe keys
def test_wide_multiprobe_keys_match_oracle_sampler():
    dims = [128, 1024, 1024, 12]
    Ws, bs = _weights(dims, 300)
    x, _, _ = synth.standardise(synth.sift_like(300, dims[0], seed=32))
    for compat, mode in ((True, "ref_int16"), (False, "full")):
        h = _hashing(dims, Ws, bs, compat=compat)
        _, probs, _ = h.forward_device(dev(x))
        p01 = probs.cpu().numpy()
        for n in (10, 128):
            for n_multi in (300, 256, 0):
                keys, nkeys = h.hash_device(dev(x), n=n, n_multi_rows=n_multi, seed=1234, row0=7)
                ko, no = oracle.row_keys(p01, n, mode, seed=1234, n_multi_rows=n_multi, row0=7)
                kd = keys.cpu().numpy().astype(np.int64)
                if mode == "full":
                    kd &= 0xFFFFFFFF
                assert np.array_equal(nkeys.cpu().numpy(), no)
                live = np.arange(n)[None, :] < no[:, None]
                assert np.array_equal(kd[live], ko[live])
                assert np.all(no[n_multi:] == 1) and (n_multi == 0 or no[:n_multi].max() > 1)


# ----------------------------------------------------------------------------- 4. streamed == fused on narrow encoders
def _stream_call(L, x, dims, packed, n, n_multi, seed, row0, key_mode, ws, act=_capi.ACT_SIGMOID):
    B, H = x.shape[0], dims[-1]
    out = dict(z=torch.empty((B, H), dtype=torch.float32, device="cuda"), p=torch.empty((B, H), dtype=torch.float32, device="cuda"),
               code=torch.empty((B,), dtype=torch.int32, device="cuda"), keys=torch.empty((B, n), dtype=torch.int32, device="cuda"),
               nkeys=torch.empty((B,), dtype=torch.int32, device="cuda"))
    args = (_capi.ptr(x), B, x.stride(0), len(dims) - 1, _capi.int_array(dims), _capi.ptr(packed), act, key_mode, n, n_multi, seed, row0,
            _capi.ptr(out["z"]), _capi.ptr(out["p"]), _capi.ptr(out["code"]), _capi.ptr(out["keys"]), _capi.ptr(out["nkeys"]))
    stream = torch.cuda.current_stream().cuda_stream
    if ws is None:
        _capi.check(L.nlsh_encode_hash(*args, stream))
    else:
        _capi.check(L.nlsh_encode_hash_stream(*args, _capi.ptr(ws), ws.numel(), stream))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _stream_pack(L, h):
    stack = [(w.float().contiguous(), None if b is None else b.float().contiguous()) for w, b in h.linear_stack()]
    dims = h.dims()
    packed = torch.empty((L.nlsh_encoder_stream_packed_floats(len(dims) - 1, _capi.int_array(dims)),), dtype=torch.float32, device="cuda")
    _capi.check(L.nlsh_encoder_stream_pack(len(dims) - 1, _capi.int_array(dims), _capi.ptr_array([w for w, _ in stack]),
                                           _capi.ptr_array([b for _, b in stack]), _capi.ptr(packed), torch.cuda.current_stream().cuda_stream))
    return packed, stack


@pytest.mark.parametrize("dims", [[25, 96, 8], [50, 64, 64, 12], [200, 256, 256, 24], [96, 320, 40, 32],
                                  [128, 600, 16], [100, 256, 256, 256, 256, 20], [128, 33, 1], [960, 256, 256, 32], [1024, 64, 7]])
def test_streamed_equals_fused_on_narrow_encoders(dims):
    L = _capi.lib()
    Ws, bs = synth.make_weights(dims, seed=7)
    x = dev(synth.glove_like(130, dims[0], seed=9))
    for compat in (True, False):
        h = _hashing(dims, Ws, bs, compat=compat)
        assert not h.streamed()
        packed_s, _keep = _stream_pack(L, h)
        ws = torch.empty((L.nlsh_encode_stream_workspace(130, len(dims) - 1, _capi.int_array(dims)),), dtype=torch.uint8, device="cuda")
        for n, n_multi, seed, row0 in ((1, 130, 0, 0), (10, 100, 99, 7), (64, 64, 5, 1000)):
            fused = _stream_call(L, x, dims, h.packed_weights(), n, n_multi, seed, row0, h.key_mode, None)
            streamed = _stream_call(L, x, dims, packed_s, n, n_multi, seed, row0, h.key_mode, ws)
            for k in fused:
                assert np.array_equal(_bits(fused[k]), _bits(streamed[k])), (k, n, n_multi)


# ----------------------------------------------------------------------------- 5. workspace-size independence
def test_outputs_do_not_depend_on_the_workspace_size():
    L = _capi.lib()
    Ws, bs = _weights(WIDE, 12)
    h = _hashing(WIDE, Ws, bs)
    x, _, _ = synth.standardise(synth.sift_like(20_000, WIDE[0], seed=12))
    xd = dev(x)
    packed = h.packed_weights()
    small = torch.empty((L.nlsh_encode_stream_workspace(1, 3, _capi.int_array(WIDE)),), dtype=torch.uint8, device="cuda")
    whole = torch.empty((L.nlsh_encode_stream_workspace(20_000, 3, _capi.int_array(WIDE)),), dtype=torch.uint8, device="cuda")
    a = _stream_call(L, xd, WIDE, packed, 10, 15_000, 42, 3, h.key_mode, small)
    b = _stream_call(L, xd, WIDE, packed, 10, 15_000, 42, 3, h.key_mode, whole)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["nkeys"][:15_000].max() > 1 and a["nkeys"][15_000:].max() == 1
    # and a capped facade workspace (several passes) gives the same keys as one pass
    h.stream_workspace_cap = 1
    k1, n1 = h.hash_device(xd, n=10, seed=42, row0=3, n_multi_rows=15_000)
    assert np.array_equal(k1.cpu().numpy(), a["keys"]) and np.array_equal(n1.cpu().numpy(), a["nkeys"])


# ----------------------------------------------------------------------------- 6. end to end
@pytest.fixture(scope="module")
def wide_corpus():
    corpus, mean, std = synth.standardise(synth.sift_like(50_000, 128, seed=61))
    queries, _, _ = synth.standardise(synth.sift_like(1000, 128, seed=synth.SEED_QUERY), mean, std)
    return corpus, queries


@pytest.mark.parametrize("compat", [True, False], ids=["int16", "full"])
def test_wide_indexer_end_to_end(wide_corpus, compat):
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    corpus, queries = wide_corpus
    Ws, bs = _weights(WIDE, 71)
    h = _hashing(WIDE, Ws, bs, compat=compat)
    mode = "ref_int16" if compat else "full"
    cg, qg = dev(corpus), dev(queries)
    ix = Indexer(h, cg, SIFT.distance, compat=compat)
    assert not ix._fuses(qg, 10, _capi.SCAN_BUCKET_TILED)
    # corpus keys = the oracle's bit rule and packing on the device's z of every row
    z, _, _ = h.forward_device(cg)
    zh = z.cpu().numpy()
    _, p01 = oracle.head_probs(zh)
    ko = oracle.pack_keys(oracle.hard_bits(p01)[:, None, :], mode)[:, 0]
    ck = ix.corpus_keys.cpu().numpy().astype(np.int64)
    if not compat:
        ck &= 0xFFFFFFFF
    assert np.array_equal(ck, ko)
    assert ix.n_buckets > 16
    # z itself against the oracle's forward on a slice (the scalar oracle is too slow for all rows)
    assert np.array_equal(_bits(zh[:4096]), _bits(oracle.mlp_forward(corpus[:4096], Ws, bs)))
    ox = oracle.OracleIndexer.from_keys(corpus, ix.corpus_keys.cpu().numpy())
    seed, k, P = 808, 10, 10
    keys, nkeys = ix.hash_device(qg, hash_times=P, seed=seed)
    kh, nh = keys.cpu().numpy().astype(np.int64), nkeys.cpu().numpy()
    key_lists = [list(set(int(v) for v in kh[i, :nh[i]])) for i in range(len(queries))]
    ores, oncl, _, oi = ox.query_with_keys(queries, key_lists, k)
    if not compat:      # compat=False: a short query returns its own candidates, not the last key's bucket (F7 is a compat quirk)
        ores = [r if oncl[i] >= k else [int(v) for v in oi[i] if v >= 0] for i, r in enumerate(ores)]
    for algo in ("query", "bucket", "tiled"):
        ix.algo = algo
        ids, ncand = ix.query(qg, k=k, hash_times=P, seed=seed)
        assert ncand == oncl, algo
        assert ids == ores, algo
        dist, idx, nc, _ = ix.query_tensors(qg, k=k, hash_times=P, seed=seed)
        assert nc.cpu().tolist() == ncand, algo
        full = [i for i in range(len(queries)) if ncand[i] >= k]
        assert full and all(idx[i].cpu().tolist() == ids[i] for i in full), algo
    ix.algo = None


# ----------------------------------------------------------------------------- 7. checkpoint round trip
def test_wide_checkpoint_round_trip(tmp_path):
    from nlsh_amd import io
    dims = [128, 1024, 1024, 16]
    Ws, bs = _weights(dims, 90)
    path = tmp_path / "wide.npz"
    np.savez(path, **{f"W{i}": w for i, w in enumerate(Ws)}, **{f"b{i}": b for i, b in enumerate(bs)})
    Wl, bl = io.load_hasher_weights(str(path))
    h = io.hashing_from_weights(Wl, bl)
    assert h.streamed() and h.dims() == dims
    x, _, _ = synth.standardise(synth.sift_like(500, 128, seed=91))
    keys, nkeys = h.hash_device(dev(x), n=1)
    _, p01 = oracle.head_probs(oracle.mlp_forward(x, Ws, bs))
    ko = oracle.pack_keys(oracle.hard_bits(p01)[:, None, :], "ref_int16")[:, 0]
    assert np.array_equal(keys.cpu().numpy()[:, 0].astype(np.int64), ko) and np.all(nkeys.cpu().numpy() == 1)
    assert len(h.hash(dev(x), 3)) == 500


# ----------------------------------------------------------------------------- 8. refusal
def test_pipeline_refuses_a_wide_encoder(wide_corpus):
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.pipeline import QueryPipeline
    corpus, queries = wide_corpus
    Ws, bs = _weights(WIDE, 71)
    h = _hashing(WIDE, Ws, bs)
    ix = Indexer(h, dev(corpus[:5000]), SIFT.distance)
    for graph in (True, False):
        with pytest.raises(_capi.NlshHipError) as e:
            QueryPipeline(ix, dev(queries[:256]), k=10, hash_times=10, graph=graph)
        assert e.value.code == _capi.E_UNSUPPORTED and "1024" in str(e.value)
    with pytest.raises(_capi.NlshHipError) as e:
        h.encode_args(10, torch.empty((1, 10), dtype=torch.int32, device="cuda"), torch.empty((1,), dtype=torch.int32, device="cuda"))
    assert e.value.code == _capi.E_UNSUPPORTED


def test_batchnorm_wide_encoder_in_train_and_eval_mode():
    """Train mode with BatchNorm runs the module's own torch forward; eval mode folds the running statistics into the streamed blob."""
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.hashings import MultivariateBernoulli
    torch.manual_seed(3)
    h = MultivariateBernoulli(MultiLayerRelu(64, [800, 800], with_batchnorm=True), 12, None)
    x = dev(synth.glove_like(512, 64, seed=5))
    h.train_mode(True)
    keys, nkeys = h.hash_device(x, n=4)
    assert keys.shape == (512, 4) and int(nkeys.min()) >= 1
    h.train_mode(False)
    z, _, _ = h.forward_device(x)
    stack = h.linear_stack()
    Ws = [w.cpu().numpy() for w, _ in stack]
    bs = [None if b is None else b.cpu().numpy() for _, b in stack]
    assert np.array_equal(_bits(z.cpu().numpy()), _bits(oracle.mlp_forward(x.cpu().numpy(), Ws, bs)))
