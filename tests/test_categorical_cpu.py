"""Categorical hashing, the parts that need no device: the numpy reference of `nlsh_probe_bins` (tests/categorical_ref.py) held against its
own second statement, the host-side refusals of the new C calls, the sizes `nlsh_logits_workspace` / `nlsh_logits_packed_floats` report,
the facade's ValueErrors and the partition trainer on a toy set."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import categorical_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {"random": cr.random_rows, "ties": cr.tie_rows, "special": cr.special_rows, "mixed": cr.mixed_rows}
NEW_CALLS = ("nlsh_logits_packed_floats", "nlsh_logits_pack", "nlsh_logits_workspace", "nlsh_encode_logits", "nlsh_probe_bins",
             "nlsh_probe_bins_budget")


@pytest.fixture(scope="module")
def L():
    from nlsh_amd import _capi
    return _capi.lib()


# ---------------------------------------------------------------------------- the reference
def test_order_bits_is_the_ieee_total_order():
    z = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38, np.inf], dtype=np.float32)
    u = cr.order_bits(z).astype(np.int64)
    assert (np.diff(u) > 0).all()                                   # strictly ascending: -0 < +0, -inf lowest, +inf highest
    assert u[0] == 0x007FFFFF and u[-1] == 0xFF800000


@pytest.mark.parametrize("kind", sorted(ROWS))
@pytest.mark.parametrize("M", [1, 2, 5, 64, 65, 300])
def test_the_two_statements_of_the_definition_agree(kind, M):
    z = ROWS[kind](9, M, seed=7 * M + len(kind))
    for P in (1, 2, 10, 64, 128):                                   # P > M included
        a = cr.table(z, P, n_multi_rows=6, fn=cr.ranked_by_sort)
        b = cr.table(z, P, n_multi_rows=6, fn=cr.ranked_by_argmax)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (kind, M, P)
        keys, nkeys, bits = a
        assert nkeys[:6].tolist() == [min(P, M)] * 6 and nkeys[6:].tolist() == [1] * 3
        past = np.arange(P)[None, :] >= nkeys[:, None]
        assert not keys[past].any() and (bits[past] == cr.NEG_INF_BITS).all()
        for r in range(9):                                            # distinct bins, each slot's logit is its bin's, bit for bit
            row = keys[r, :nkeys[r]]
            assert len(set(row.tolist())) == len(row) and np.array_equal(z[r, row].view(np.uint32), bits[r, :nkeys[r]])


def test_equal_rows_give_the_bins_in_index_order_and_signed_zeros_split():
    keys, nkeys, _ = cr.table(cr.equal_rows(3, 100), 10)
    assert (keys == np.arange(10)[None, :]).all() and nkeys.tolist() == [10] * 3
    z = np.array([[-0.0, 0.0, -0.0, 0.0, -np.inf, np.inf]], dtype=np.float32)
    assert cr.table(z, 6)[0].tolist() == [[5, 1, 3, 0, 2, 4]]


@pytest.mark.parametrize("M", [3, 64, 300])
def test_the_budget_walk_equals_the_prefix_sum_cut(M):
    z = cr.mixed_rows(12, M, seed=M)
    uniq, offsets = cr.bin_csr(M, seed=M + 5)
    stopped = 0
    for P in (1, 10, 128):
        full = cr.table(z, P, n_multi_rows=9)
        for budget in (1, 3, 40, 5000, cr.INT32_MAX):
            a, b = cr.walk(*full, uniq, offsets, budget), cr.cut(*full, uniq, offsets, budget)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (M, P, budget)
            assert (a[1] >= 1).all() and np.array_equal(a[0][:, 0], full[0][:, 0])             # slot 0 is always kept
            stopped += int((a[1] < full[1]).sum())
        unb = cr.cut(*full, uniq, offsets, cr.INT32_MAX)
        assert all(np.array_equal(x, y) for x, y in zip(unb[:3], full))
        empty = cr.cut(*full, np.zeros((0,), np.int32), np.zeros((1,), np.int32), 1)
        assert all(np.array_equal(x, y) for x, y in zip(empty[:3], full)) and not empty[3].any()
    assert stopped


# ---------------------------------------------------------------------------- exports
def test_header_declares_the_calls_and_the_abi_is_still_4(L):
    from nlsh_amd import _capi
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    for name in NEW_CALLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _capi.SYMBOLS and hasattr(L, name), name
    assert int(re.search(r"#define NLSH_MAX_BINS (\d+)", header).group(1)) == _capi.MAX_BINS == _capi.MAX_STREAM_WIDTH == 4096
    makefile = open(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "csrc", "Makefile")).read()
    assert "probe_categorical.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, re.M).group(1)
    assert int(re.search(r"#define NLSH_ABI_VERSION (\d+)", header).group(1)) == 4 and L.nlsh_abi_version() == 4


# ---------------------------------------------------------------------------- nlsh_probe_bins[_budget]: host-side checks
def _probe(L, logits=True, keys=True, nkeys=True, uniq=True, offsets=True, n=8, M=100, stride=None, P=10, n_multi=None, n_buckets=5,
           budget=None):
    """One of the two calls (budget None: the unbudgeted one) with pointers into a small host buffer: every call here must be answered
    before any of them is used."""
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255
    p = lambda on: a if on else None   # noqa: E731
    head = (p(logits), M if stride is None else stride, n, M, P, n if n_multi is None else n_multi)
    if budget is None:
        return L.nlsh_probe_bins(*head, p(keys), p(nkeys), None, None)
    return L.nlsh_probe_bins_budget(*head, p(uniq), p(offsets), n_buckets, budget, p(keys), p(nkeys), None, None, None)


@pytest.mark.parametrize("budget", [None, 100])
def test_probe_bins_refusals(L, budget):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731
    for missing in ("logits", "keys", "nkeys"):
        assert _probe(L, budget=budget, **{missing: False}) == _capi.E_INVALID, missing
        assert "null pointer" in err()
    assert _probe(L, budget=budget, n=-1) == _capi.E_INVALID and "n=-1" in err()
    assert _probe(L, budget=budget, M=100, stride=99) == _capi.E_INVALID and "logits_stride=99" in err() and "M=100" in err()
    for M in (0, -3, 4097):
        assert _probe(L, budget=budget, M=M, stride=8192) == _capi.E_UNSUPPORTED
        assert "NLSH_MAX_BINS" in err() and f"M={M}" in err()
    for P in (0, 129, -1):
        assert _probe(L, budget=budget, P=P) == _capi.E_UNSUPPORTED
        assert "NLSH_MAX_ENCODE_PROBES" in err() and f"n_probes={P}" in err()
    assert _probe(L, budget=budget, n=0) == _capi.OK                # an empty batch: OK without a launch, pointers or not
    assert _probe(L, budget=budget, n=0, logits=False, keys=False, nkeys=False, uniq=False, offsets=False, n_buckets=0) == _capi.OK
    assert _probe(L, budget=budget, n=0, M=5000, stride=8192) == _capi.E_UNSUPPORTED


def test_probe_bins_budget_refusals_of_its_own(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731
    for budget in (0, -1, -(2 ** 31)):
        assert _probe(L, budget=budget) == _capi.E_INVALID and f"budget={budget}" in err()
    for nb in (-1, -70000):
        assert _probe(L, budget=5, n_buckets=nb) == _capi.E_INVALID and f"n_buckets={nb}" in err()
    for missing in ("uniq", "offsets"):
        assert _probe(L, budget=5, **{missing: False}) == _capi.E_INVALID, missing
        assert "null pointer" in err() and "n_buckets=5" in err()
    assert _probe(L, budget=5, n=0, uniq=False) == _capi.E_INVALID   # the index arrays are checked for an empty batch too
    assert _probe(L, budget=0, n=0) == _capi.E_INVALID


# ---------------------------------------------------------------------------- the logits forward: sizes and host-side checks
def _arr(dims):
    from nlsh_amd import _capi
    return _capi.int_array(dims)


def test_logits_blob_and_workspace_sizes(L):
    up = lambda x, m: (x + m - 1) // m * m   # noqa: E731
    for dims in ([128, 256], [128, 256, 256], [25, 633, 100], [100, 64, 4096], [96, 1024, 1000], [1024, 512, 1], [8, 4096, 4096, 7]):
        nl = len(dims) - 1
        blob = sum(up(dims[l + 1], 32) * up(dims[l], 8) + up(dims[l + 1], 32) for l in range(nl))     # the streamed layout: W then b per layer
        assert L.nlsh_logits_packed_floats(nl, _arr(dims)) == blob, dims
        if dims[-1] <= 32:                                           # ... which the streamed hashing form shares where it takes the shape
            assert L.nlsh_encoder_stream_packed_floats(nl, _arr(dims)) == blob
        ws = max((up(h, 32) for h in dims[1:-1]), default=0)
        per_row = min(2, nl - 1) * ws + (up(dims[-1], 32) if dims[-1] % 32 else 0)
        for rows, tiles in ((0, 1), (1, 1), (128, 1), (129, 2), (4097, 33)):
            assert L.nlsh_logits_workspace(rows, nl, _arr(dims)) == max(tiles * 128 * per_row * 4, 16), (dims, rows)


def test_logits_shape_refusals(L):
    from nlsh_amd import _capi
    bad = ([128, 4097], [128, 256, 5000], [128, 4097, 16], [1025, 64], [128, 0], [0, 16], [128, -4, 16])
    for dims in bad:
        nl = len(dims) - 1
        assert L.nlsh_logits_packed_floats(nl, _arr(dims)) == -1, dims
        assert L.nlsh_logits_workspace(128, nl, _arr(dims)) == 0, dims
    assert L.nlsh_logits_packed_floats(0, _arr([128])) == -1 and L.nlsh_logits_packed_floats(9, _arr([8] * 10)) == -1
    assert L.nlsh_logits_packed_floats(1, None) == -1 and L.nlsh_logits_workspace(-1, 1, _arr([128, 256])) == 0
    # the hashing calls keep refusing an output layer wider than 32
    assert L.nlsh_encoder_stream_packed_floats(1, _arr([128, 256])) == -1 and L.nlsh_encoder_packed_floats(1, _arr([128, 256])) == -1
    assert L.nlsh_encode_stream_workspace(128, 2, _arr([128, 256, 33])) == 0
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255
    assert L.nlsh_encode_hash_stream(a, 4, 128, 1, _arr([128, 256]), a, 0, 1, 1, 4, 0, 0, None, None, None, a, a, a, 1 << 20, None) == _capi.E_UNSUPPORTED
    assert "hash_size 256" in L.nlsh_last_error().decode()


def _logits(L, x=True, packed=True, out=True, ws=True, n=4, dims=(128, 256, 100), x_stride=None, out_stride=None, ws_bytes=1 << 20, ws_shift=0):
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255
    p = lambda on: a if on else None   # noqa: E731
    return L.nlsh_encode_logits(p(x), n, dims[0] if x_stride is None else x_stride, len(dims) - 1, _arr(dims), p(packed), p(out),
                                dims[-1] if out_stride is None else out_stride, (a + ws_shift) if ws else None, ws_bytes, None)


def test_encode_logits_refusals(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731
    for missing in ("x", "packed", "out", "ws"):
        assert _logits(L, **{missing: False}) == _capi.E_INVALID and "null pointer" in err(), missing
    assert _logits(L, n=-1) == _capi.E_INVALID and "n=-1" in err()
    assert _logits(L, x_stride=127) == _capi.E_INVALID and "x_stride 127" in err()
    assert _logits(L, out_stride=99) == _capi.E_INVALID and "logits_stride 99" in err()
    assert _logits(L, ws_shift=4) == _capi.E_INVALID and "16-byte aligned" in err()
    assert _logits(L, ws_bytes=1000) == _capi.E_WORKSPACE and "workspace 1000 B" in err()
    assert _logits(L, dims=(128, 256, 4097)) == _capi.E_UNSUPPORTED and "NLSH_MAX_BINS" in err()
    assert _logits(L, dims=(128, 5000, 16)) == _capi.E_UNSUPPORTED
    assert _logits(L, n=0) == _capi.OK and _logits(L, n=0, x=False, packed=False, out=False, ws=False, ws_bytes=0) == _capi.OK
    assert _logits(L, n=0, dims=(128, 256, 4097)) == _capi.E_UNSUPPORTED
    null = _capi.ptr_array([None])
    assert L.nlsh_logits_pack(1, _arr([128, 256]), null, null, None, None) == _capi.E_INVALID and "null pointer" in err()
    assert L.nlsh_logits_pack(1, _arr([128, 5000]), null, null, None, None) == _capi.E_UNSUPPORTED


# ---------------------------------------------------------------------------- the Python surface
@pytest.fixture()
def host_modules(monkeypatch):
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)      # no GPU here; what is tested is host logic


def test_categorical_constructor_and_probes(host_modules, monkeypatch):
    from nlsh_amd import _capi, hashings
    from nlsh_amd.encoders import MultiLayerRelu
    monkeypatch.syspath_prepend(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "compat"))   # the reference's import names
    import nlsh.hashings as compat_hashings
    assert compat_hashings.Categorical is hashings.Categorical
    for bad in (0, -1, 4097):
        with pytest.raises(ValueError, match="hash_size"):
            hashings.Categorical(MultiLayerRelu(8, [16]), bad, None)
    h = hashings.Categorical(MultiLayerRelu(8, [16]), 100, lambda a, b: (a - b).abs().sum(1))
    assert h.output_dim == 100 and h.key_mode == _capi.KEY_FULL and h.probes == "ranked" and h.dims() == [8, 16, 100]
    assert not hasattr(h, "encode_args") and not hasattr(h, "ranked_encode_args")          # Indexer takes the two-step route
    assert sorted(dict(h._hasher.named_children())) == ["_encoder", "output_layer"]        # the reference module's child names
    assert h.distance(torch.ones(2, 3), torch.zeros(2, 3)).tolist() == [3.0, 3.0]
    h.probes = "ranked"
    with pytest.raises(ValueError, match="Bernoulli"):
        h.probes = "sampled"
    with pytest.raises(ValueError, match="probes"):
        h.probes = "nonsense"
    x = torch.zeros(3, 8)
    for call in (lambda: h.hash(x, probes="sampled"), lambda: h.hash_device(x, n=4, probes="sampled")):
        with pytest.raises(ValueError, match="Bernoulli"):
            call()
    assert h.probes == "ranked"
    for bad in (0, -2):
        with pytest.raises(ValueError, match="positive"):
            h.hash_device(x, n=bad)
    with pytest.raises(_capi.NlshHipError) as e:                                           # valid arguments reach the device requirement
        h.hash_device(x, n=4, probes="ranked")
    assert e.value.code == _capi.E_INVALID
    with pytest.raises(_capi.NlshHipError) as e:
        h.hash_device(x, n=_capi.MAX_ENCODE_PROBES + 1)
    assert e.value.code == _capi.E_UNSUPPORTED
    h.train_mode(True)                                                                     # train mode: the autograd forward
    p = h.predict(torch.randn(5, 8))
    assert p.requires_grad and p.shape == (5, 100) and torch.allclose(p.sum(1), torch.ones(5), atol=1e-5)
    assert len(list(h.parameters())) == 4


def test_state_dicts_interchange_and_a_batchnorm_encoder_in_train_mode_is_refused(host_modules, tmp_path):
    from nlsh_amd import _capi, hashings
    from nlsh_amd.encoders import MultiLayerRelu
    a = hashings.Categorical(MultiLayerRelu(8, [16]), 12, None)
    b = hashings.Categorical(MultiLayerRelu(8, [16]), 12, None)
    torch.save(a._hasher.state_dict(), tmp_path / "a_state.pt")
    b.load_state(str(tmp_path / "a_state.pt"))
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert sorted(a._hasher.state_dict()) == sorted(hashings.MultivariateBernoulli(MultiLayerRelu(8, [16]), 12, None)._hasher.state_dict())

    class BnEncoder(torch.nn.Module):
        output_dim = 16

        def __init__(self):
            super().__init__()
            self.lin, self.bn = torch.nn.Linear(8, 16), torch.nn.BatchNorm1d(16)

        def forward(self, x):
            return torch.relu(self.bn(self.lin(x)))
    h = hashings.Categorical(BnEncoder(), 12, None)
    h.train_mode(True)
    assert h._needs_train_forward()
    x = torch.zeros(3, 8)
    with pytest.raises(_capi.NlshHipError, match="eval mode") as e:
        h.logits_device(_FakeDevice(x))
    assert e.value.code == _capi.E_UNSUPPORTED


class _FakeDevice:
    """A tensor stand-in that says it is on the device: the train-mode refusal comes before anything reads it."""
    def __init__(self, t):
        self.shape, self.dtype = t.shape, t.dtype
        self.device = torch.device("cuda", 0)


def test_indexer_delegates_the_budget_to_the_hasher(host_modules):
    from nlsh_amd.indexer import Indexer
    seen = {}

    class Stub:
        probes, key_mode = "ranked", 1

        def hash_budget_device(self, x, n, n_multi_rows, uniq_keys, offsets, n_buckets, budget, out=None):
            seen.update(n=n, n_multi_rows=n_multi_rows, uniq_keys=uniq_keys, offsets=offsets, n_buckets=n_buckets, budget=budget, out=out)
            return "keys", "nkeys", "ncand"
    ix = Indexer.__new__(Indexer)
    ix._hashing, ix.compat, ix.metric = Stub(), True, "l2"
    ix.uniq_keys, ix.offsets, ix.n_buckets = "U", "O", 7
    ix._as_queries = lambda q: q
    x = torch.zeros(2500, 8)
    assert ix._hash_budget(x, 1000, 12, 345) == ("keys", "nkeys", "ncand")
    assert seen == dict(n=12, n_multi_rows=2000, uniq_keys="U", offsets="O", n_buckets=7, budget=345, out=None)   # compat: full batches only
    assert ix.hash_device(x, 1000, 12, candidate_budget=9) == ("keys", "nkeys") and seen["budget"] == 9


def test_pipelines_and_sharded_indexes_refuse_a_categorical_hasher(host_modules):
    from nlsh_amd import _capi, hashings
    from nlsh_amd.distributed import ShardedIndexer
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.pipeline import QueryPipeline
    h = hashings.Categorical(MultiLayerRelu(8, [16]), 12, None)
    ix = Indexer.__new__(Indexer)
    ix._hashing, ix.refine, ix.storage = h, None, "float32"
    for graph in (True, False):
        with pytest.raises(_capi.NlshHipError, match="Categorical") as e:
            QueryPipeline(ix, torch.zeros(4, 8), graph=graph)
        assert e.value.code == _capi.E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="Categorical"):
        ShardedIndexer(h, torch.zeros(4, 8), None, id_base=0)


# ---------------------------------------------------------------------------- the partition trainer
def test_partition_targets_are_one_hot_or_the_neighbour_histogram():
    from nlsh_amd.training import partition_targets
    labels = torch.tensor([0, 2, 2, 1])
    assert partition_targets(labels, 3).tolist() == [[1, 0, 0], [0, 0, 1], [0, 0, 1], [0, 1, 0]]
    knn = torch.tensor([[1, 2, 3], [0, 2, 3], [1, 0, 3], [0, 1, 2]])
    soft = partition_targets(labels, 3, knn, soft_k=2)                # first two neighbours only
    assert torch.allclose(soft, torch.tensor([[0, 0, 1.0], [.5, 0, .5], [.5, 0, .5], [.5, 0, .5]]))
    assert torch.allclose(partition_targets(labels, 3, knn, soft_k=3).sum(1), torch.ones(4))


@pytest.mark.parametrize("soft", [False, True])
def test_fit_partition_lowers_its_loss_on_a_toy_set(host_modules, soft):
    """200 rows in 4 well-separated blobs, labels = the blob: cross-entropy starts near ln 4 and the fit brings it far down."""
    from nlsh_amd import hashings
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.training import fit_partition
    torch.manual_seed(0)
    labels = torch.arange(200) % 4
    centres = torch.tensor([[4.0, 0, 0, 0, 0, 0], [0, 4.0, 0, 0, 0, 0], [0, 0, 4.0, 0, 0, 0], [0, 0, 0, 4.0, 0, 0]])
    x = centres[labels] + 0.3 * torch.randn(200, 6)
    knn = None
    if soft:                                                          # exact neighbours of the toy set (torch, host)
        knn = torch.cdist(x, x).fill_diagonal_(float("inf")).topk(5, largest=False).indices
    h = hashings.Categorical(MultiLayerRelu(6, [16]), 4, None)
    losses = fit_partition(h, x, labels, knn=knn, soft_k=5, n_steps=150, batch_size=50, learning_rate=1e-2, seed=1)
    assert len(losses) == 150 and all(np.isfinite(losses))
    first, last = np.mean(losses[:5]), np.mean(losses[-5:])
    assert first > 0.8 and last < 0.25 * first, (first, last)
    assert not h._hasher.training                                     # left in eval mode
    h.train_mode(True)
    assert float((h.predict(x).argmax(1) == labels).float().mean()) >= 0.98
