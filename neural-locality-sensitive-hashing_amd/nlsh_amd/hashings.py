"""Learnable hash function with the reference's `MultivariateBernoulli` surface
(nlsh/hashings.py:11-92), backed by the fused gfx950 `encode_hash` kernel.

`hash()` / `predict()` (eval mode) run ONE HIP launch: MLP forward on fp32 MFMA, sigmoid/tanh,
`> 0.5` bits, MSB-first packing, Philox multi-probe sampling and per-row de-duplication, with no
device->host copy of codes.  `hash_device()` is the device-resident form `Indexer` uses.
Encoders with a hidden layer wider than `_capi.MAX_WIDTH` (632) are "streamed": they hash through `nlsh_encode_hash_stream`
(one GEMM launch per layer, activations in a workspace the hashing owns, then the same epilogue), up to `_capi.MAX_STREAM_WIDTH`.
`probes="ranked"` (attribute, constructor keyword or per call) replaces the Philox draws by the n most probable codes in descending
probability (`nlsh_probe_ranked` on the encode's own z and hard code: two launches, no seed, n distinct codes; `Indexer` has an opt-in
one-call form of the whole ranked batch, `ranked_encode_args`); "sampled" is the default.
`Categorical` (nlsh/hashings.py:95-139) is the other family: a softmax over M bins, bucket = argmax bin, multi-probe = the next most
probable bins (`nlsh_encode_logits` + `nlsh_probe_bins`).  Both share `_DeviceHashing`: weights, repacking, workspaces.
There is no CPU fallback: a missing library or a non-device tensor raises.
"""
import itertools
from typing import List, Set

import torch
import torch.nn as nn

from . import _capi


class _Hasher(nn.Module):
    """encoder -> Linear(hash_size) -> sigmoid | tanh; same child names as the reference module
    (hashings.py:13-27: `_encoder`, `output_layer`) so state dicts interchange."""

    def __init__(self, encoder, hash_size, tanh_output=False):
        super().__init__()
        self._encoder = encoder
        self._tanh_output = tanh_output
        self.output_layer = nn.Linear(encoder.output_dim, hash_size)

    def forward(self, x):  # stock autograd path: training only (out of the hot path)
        z = self.output_layer(self._encoder(x))
        return torch.tanh(z) if self._tanh_output else torch.sigmoid(z)


class _DeviceHashing:
    """What the hash families share: the reference surface around `self._hasher` (an nn.Module with `_encoder` and `output_layer`),
    the layer stack, the packed weight blob with its repack-on-change signature, and the per-stream workspace of the layer-GEMM
    forms.  A family names its pack calls (`_pack_calls`) and says whether its forward runs the layer GEMMs (`streamed`)."""
    # bytes of device memory a layer-GEMM forward's workspace may take per (device, stream): the C side makes as many passes over
    # the rows as this needs (at 1024-wide layers, 8.3 KB per row: ~32k rows per pass)
    stream_workspace_cap = 256 << 20

    def _init_hasher(self, encoder, hash_size, distance_func, hasher, seed):
        self._encoder = encoder
        self._hash_size = hash_size
        self._distance_func = distance_func  # code-space distance: training only (hashings.py:33-34)
        self._hasher = hasher.cuda()
        self._seed = int(seed)
        self._calls = itertools.count()
        self._packed = None
        self._packed_sig = None

    # ------------------------------------------------------------------ reference surface
    @property
    def distance(self):
        return self._distance_func

    @property
    def output_dim(self):
        return self._hash_size

    def parameters(self):
        return self._hasher.parameters()

    def train_mode(self, on):
        self._hasher.train(bool(on))

    def save(self, base_name):
        """TorchScript `_cpu.pt` / `_gpu.pt` like hashings.py:53-57, plus a plain state dict
        (`_state.pt`), which `load_state` reads back (the reference has no loader: :58)."""
        torch.save(self._hasher.state_dict(), base_name + "_state.pt")
        for suffix, module in (("_cpu.pt", self._hasher.cpu()), ("_gpu.pt", self._hasher.cuda())):
            torch.jit.save(torch.jit.script(module), base_name + suffix)

    def load_state(self, path):
        self._hasher.load_state_dict(torch.load(path, map_location="cpu"))
        self._hasher.cuda()
        self._packed_sig = None

    # ------------------------------------------------------------------ internals
    def linear_stack(self):
        stack = list(self._encoder.linear_stack())
        ol = self._hasher.output_layer
        stack.append((ol.weight.detach(), None if ol.bias is None else ol.bias.detach()))
        return stack

    def dims(self):
        stack = self.linear_stack()
        return [stack[0][0].shape[1]] + [w.shape[0] for w, _ in stack]

    def _weights_signature(self):
        """(name, storage address, version counter) of every parameter and buffer of the hasher: changes whenever an optimiser step, a
        `load_state_dict`, a `.cuda()`, a reassigned or a newly registered parameter / buffer changes what the packed blob was built
        from.  Called on every hashing call, so it walks a cached list of the modules' own `_parameters` / `_buffers` dicts (whatever
        they hold NOW: `register_buffer`, `parametrize` or an assignment on an existing module is seen through the dict) instead of
        `module.parameters()` -- the recursive module walk cost 30 us per call, a third of the host time of a pipelined batch (r04,
        cProfile of `QueryPipeline.submit`).  The list itself is rebuilt when the module tree changed shape (a submodule added,
        removed or swapped: the count and identities of the `_modules` entries are part of the cache key)."""
        cached = self.__dict__.get("_sig_slots")
        if cached is not None and cached[0] is self._hasher:
            for md, n, ids in cached[2]:                          # every module's child table: same length, same child objects
                if len(md) != n or tuple(map(id, md.values())) != ids:
                    cached = None
                    break
        if cached is None or cached[0] is not self._hasher:           # a replaced `_hasher` module gets its own walk
            mods = list(self._hasher.modules())
            cached = self._sig_slots = (self._hasher, [d for m in mods for d in (m._parameters, m._buffers)],
                                        [(m._modules, len(m._modules), tuple(map(id, m._modules.values()))) for m in mods])
        sig = []
        for d in cached[1]:
            for name, t in d.items():
                sig.append((name, None) if t is None else (name, t.data_ptr(), t._version))
        return tuple(sig)

    def packed_weights(self):
        """MFMA-fragment-ordered weight blob on the device (the streamed form's own layout for a streamed encoder); repacked when a
        parameter changes."""
        sig = self._weights_signature()
        if self._packed is not None and sig == self._packed_sig:
            return self._packed
        L = _capi.lib()
        stack = [(w.float().contiguous(), None if b is None else b.float().contiguous()) for w, b in self.linear_stack()]
        dev = stack[0][0].device
        if dev.type != "cuda":
            raise _capi.NlshHipError(_capi.E_INVALID, "hasher weights are not on the GPU; there is no CPU path")
        dims = self.dims()
        count, pack = self._pack_calls(L)
        n_floats = count(len(stack), _capi.int_array(dims))
        if n_floats < 0:
            _capi.check(_capi.E_UNSUPPORTED)
        packed = torch.empty((n_floats,), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(pack(len(stack), _capi.int_array(dims), _capi.ptr_array([w for w, _ in stack]),
                         _capi.ptr_array([b for _, b in stack]), _capi.ptr(packed), stream))
        self._packed, self._packed_sig, self._keep = packed, sig, stack
        return packed

    def _needs_train_forward(self):
        """Train mode changes the forward only for encoders with BatchNorm (batch statistics instead of the running ones the
        fused kernel folds into its weights); the plain Linear+ReLU stacks compute the same function in both modes."""
        return self._hasher.training and any(isinstance(m, nn.modules.batchnorm._BatchNorm) for m in self._hasher.modules())

    def _stream_workspace(self, L, dims, rows, device, stream, size=None):
        """A layer-GEMM forward's workspace for `rows` rows on (device, stream), capped at `stream_workspace_cap` (at least one row
        tile): one buffer per stream, so that calls on two streams never share one; grown, never shrunk.  `size`: the form's
        workspace query (default: the streamed hashing form's)."""
        size = size or L.nlsh_encode_stream_workspace
        want = size(max(rows, 1), len(dims) - 1, _capi.int_array(dims))
        floor = size(1, len(dims) - 1, _capi.int_array(dims))
        if want == 0 or floor == 0:
            raise _capi.NlshHipError(_capi.E_UNSUPPORTED, f"streamed encoder {dims}: outside the form's limits")
        want = max(min(want, self.stream_workspace_cap), floor)
        pool = self.__dict__.setdefault("_stream_ws", {})
        key = (device.index, stream)
        ws = pool.get(key)
        if ws is None or ws.numel() < want:
            ws = pool[key] = torch.empty((want,), dtype=torch.uint8, device=device)
        return ws


class MultivariateBernoulli(_DeviceHashing):
    _Hasher = _Hasher
    # multi-probe mode of hash() / hash_device(): "sampled" = the reference's Bernoulli(p) draws (Philox stream keyed by the seed),
    # "ranked" = the n most probable codes in descending probability (include/nlsh_hip.h, nlsh_probe_ranked).  A call's `probes=`
    # keyword overrides it for that call.
    probes = "sampled"

    def __init__(self, encoder, hash_size, distance_func, tanh_output=False, compat=True, seed=0, probes="sampled"):
        self.probes = _capi.probe_mode(probes)
        if not 1 <= hash_size <= _capi.MAX_HASH_BITS:
            raise ValueError(f"hash_size must be in [1, {_capi.MAX_HASH_BITS}], got {hash_size}")
        self._tanh_output = tanh_output
        # compat=True: bucket keys wrap to int16 exactly like nlsh/utils.pyx:7-15
        self.key_mode = _capi.KEY_REF_INT16 if compat else _capi.KEY_FULL
        self._init_hasher(encoder, hash_size, distance_func, _Hasher(encoder, hash_size, tanh_output), seed)

    def predict(self, x):
        """Module output [B, H].  Eval mode: HIP kernel.  Train mode: autograd forward (the
        training losses need gradients; training is outside the query-time hot path)."""
        if self._hasher.training:
            return self._hasher(x)
        return self._run(x, 1, want_probs=True)[2]

    def hash(self, query_vectors, n=1, probes=None) -> List[Set[int]]:
        """hashings.py:66-92: list of B sets of bucket keys (1 hard + n-1 sampled probes; `probes="ranked"`: the n most probable codes).
        Like the reference, the forward runs in whatever mode the module is in (`train_mode`): see `_run_train_mode`."""
        probes = _capi.probe_mode(probes, self.probes)
        if n < 1:
            raise ValueError(f"`n` should be positive integer, but got {n}")
        keys, nkeys, _ = self._run(query_vectors, n, probes=probes)
        return keys_to_sets(keys, nkeys, self.key_mode)

    # ------------------------------------------------------------------ device-resident form
    def hash_device(self, x, n=1, n_multi_rows=None, seed=None, row0=0, out=None, probes=None):
        """-> (keys int32 [B, n] distinct, first-occurrence order; nkeys int32 [B]) on the device.

        Rows >= n_multi_rows are single-probe (Indexer.hash's trailing-batch rule).  `seed`
        defaults to a per-call stream (base seed + call counter): identical on every rank.
        `probes` ("sampled" | "ranked", None = the hasher's `probes` attribute): ranked keys are a function of the row alone,
        `seed` and `row0` are accepted and ignored.
        """
        probes = _capi.probe_mode(probes, self.probes)
        if n < 1:
            raise ValueError(f"`n` should be positive integer, but got {n}")
        keys, nkeys, _ = self._run(x, n, n_multi_rows=n_multi_rows, seed=seed, row0=row0, out=out, probes=probes)
        return keys, nkeys

    def forward_device(self, x):
        """-> (z [B,H], probs [B,H], code uint32-as-int32 [B]) in one launch (tests / eval flow)."""
        B = x.shape[0]
        z = torch.empty((B, self._hash_size), dtype=torch.float32, device=x.device)
        code = torch.empty((B,), dtype=torch.int32, device=x.device)
        _, _, probs = self._run(x, 1, want_probs=True, z_out=z, code_out=code)
        return z, probs, code

    def encode_device(self, x):
        """-> (z [B,H], code uint32-as-int32 [B]): the one-probe encode launch of the ranked mode alone (LDS-resident or streamed form),
        for callers that probe behind it themselves (`Indexer`'s candidate budget: `nlsh_probe_ranked_budget` needs the index's CSR
        arrays).  No seed is drawn; a BatchNorm encoder in train mode is refused as for `probes="ranked"`."""
        B = x.shape[0]
        z = torch.empty((B, self._hash_size), dtype=torch.float32, device=x.device)
        code = torch.empty((B,), dtype=torch.int32, device=x.device)
        self._run(x, 1, z_out=z, code_out=code, probes="ranked")
        return z, code

    # ------------------------------------------------------------------ internals
    def streamed(self):
        """True when a hidden layer is wider than the LDS-resident forms take (`_capi.MAX_WIDTH`): the encoder hashes through the
        streamed form, which no pipelined batch slot or fused query call takes.  Asked on every hashing / query call: cached on the
        weights' signature (a width changes only with a new parameter) instead of walking the layer stack each time."""
        sig = self._weights_signature()
        cached = self.__dict__.get("_streamed_for")
        if cached is None or cached[0] != sig:
            cached = self._streamed_for = (sig, max(self.dims()[1:-1], default=0) > _capi.MAX_WIDTH)
        return cached[1]

    def _pack_calls(self, L):
        return ((L.nlsh_encoder_stream_packed_floats, L.nlsh_encoder_stream_pack) if self.streamed()
                else (L.nlsh_encoder_packed_floats, L.nlsh_encoder_pack))

    def encode_args(self, n, keys, nkeys):
        """Fixed part of an `nlsh_encode_hash` call that fills a caller-owned key table (weights as they are NOW):
        (n_layers, dims array, packed weights ptr, act, key_mode, n_probes) and the output pointers, as plain values
        for callers that launch many batches (nlsh_amd/pipeline.py).  A streamed encoder has no such call, and neither has a ranked
        hasher (its keys take a second launch): NlshHipError(E_UNSUPPORTED)."""
        if self.probes == "ranked":
            raise _capi.NlshHipError(_capi.E_UNSUPPORTED, "probes='ranked': the keys come from nlsh_probe_ranked behind the encode "
                                                          "(no fused / pipelined encode launch); batch slots are sampled-only")
        dims = self.dims()
        if self.streamed():
            raise _capi.NlshHipError(_capi.E_UNSUPPORTED, f"hidden width {max(dims[1:-1])} > {_capi.MAX_WIDTH}: the encoder hashes "
                                                          "through the streamed form only (no fused / pipelined encode launch)")
        self._dims_arr = _capi.int_array(dims)
        packed = self.packed_weights()
        return ((len(dims) - 1, self._dims_arr, packed.data_ptr(), _capi.ACT_TANH if self._tanh_output else _capi.ACT_SIGMOID,
                 self.key_mode, n), (None, None, None, keys.data_ptr(), nkeys.data_ptr()))

    def ranked_encode_args(self, n):
        """`encode_args`' sibling for the ranked mode's one-call form (`nlsh_query_batch_ranked`): the descriptor's encoder fields
        (n_layers, dims array, packed weights ptr, act, key_mode, n = width of the ranked key table) with the weights as they are NOW.
        The call's encode launch makes one probe into the call's scratch, so there are no output pointers; no seed is involved.  A
        streamed encoder has no such call: NlshHipError(E_UNSUPPORTED)."""
        dims = self.dims()
        if self.streamed():
            raise _capi.NlshHipError(_capi.E_UNSUPPORTED, f"hidden width {max(dims[1:-1])} > {_capi.MAX_WIDTH}: the encoder hashes "
                                                          "through the streamed form only (no one-call ranked batch)")
        self._dims_arr = _capi.int_array(dims)
        packed = self.packed_weights()
        return (len(dims) - 1, self._dims_arr, packed.data_ptr(), _capi.ACT_TANH if self._tanh_output else _capi.ACT_SIGMOID, self.key_mode, n)

    def next_seed(self):
        return (self._seed + 0x9E3779B97F4A7C15 * (next(self._calls) + 1)) & 0xFFFFFFFFFFFFFFFF

    def _run_train_mode(self, x, n, n_multi_rows, want_probs, out):
        """`hash()` / `hash_device()` while the module is in TRAIN mode and has BatchNorm layers: the reference's `hash` runs
        `self._hasher(query_vectors)` in the module's current mode (nlsh/hashings.py:66-67; nlsh/trainers/proposed.py:101-104
        calls it between optimiser steps, in train mode), i.e. with BATCH statistics and a running-statistics update.  That
        forward cannot be folded into the fused kernel's weights, and training is outside the query-time hot path, so this
        branch mirrors the reference op for op on the device: the module's own forward, `> 0.5`, `torch.bernoulli` draws (the
        global torch RNG, as `Bernoulli.sample` uses), then `nlsh_pack_codes` and a first-occurrence de-duplication per row."""
        from .utils import pack_codes
        with torch.no_grad():
            probs = self._hasher(x)
        p01 = probs / 2. + 0.5 if self._tanh_output else probs
        base = (p01 > 0.5).int().unsqueeze(1)
        if n > 1:
            sampled = torch.bernoulli(p01.unsqueeze(0).expand(n - 1, -1, -1)).int().permute(1, 0, 2)
            codes = torch.cat((base, sampled), dim=1)
        else:
            codes = base
        B = x.shape[0]
        every = pack_codes(codes.contiguous(), "ref_int16" if self.key_mode == _capi.KEY_REF_INT16 else "full", device=x.device)
        earlier = torch.tril(torch.ones((n, n), dtype=torch.bool, device=x.device), diagonal=-1)
        dup = ((every[:, :, None] == every[:, None, :]) & earlier[None]).any(2)
        if n_multi_rows is not None and n > 1:      # Indexer.hash's trailing-batch rule: rows >= n_multi_rows are single-probe
            dup[int(n_multi_rows):, 1:] = True
        order = torch.argsort(dup.to(torch.int8), dim=1, stable=True)
        keys_t, nkeys_t = torch.gather(every, 1, order).contiguous(), (~dup).sum(1).to(torch.int32)
        if out is not None:
            out[0].copy_(keys_t)
            out[1].copy_(nkeys_t)
            keys_t, nkeys_t = out
        return keys_t, nkeys_t, (probs if want_probs else None)

    def _run(self, x, n, n_multi_rows=None, seed=None, row0=0, want_probs=False, z_out=None, code_out=None, out=None, probes="sampled"):
        if x.device.type != "cuda":
            raise _capi.NlshHipError(_capi.E_INVALID, "encode_hash needs a device tensor; there is no CPU path")
        ranked = probes == "ranked"
        if self._needs_train_forward():
            if ranked:
                raise _capi.NlshHipError(_capi.E_UNSUPPORTED, "probes='ranked' needs eval mode for BatchNorm encoders (train_mode(False)): "
                                                              "the train-mode forward has no z")
            if z_out is not None or code_out is not None:
                raise _capi.NlshHipError(_capi.E_UNSUPPORTED, "forward_device() needs eval mode for BatchNorm encoders (train_mode(False))")
            if x.dtype != torch.float32:
                x = x.float()
            return self._run_train_mode(x.detach(), n, n_multi_rows, want_probs, out)
        if n > _capi.MAX_ENCODE_PROBES:
            raise _capi.NlshHipError(_capi.E_UNSUPPORTED, f"hash_times={n} > {_capi.MAX_ENCODE_PROBES}")
        L = _capi.lib()
        x = x.detach()
        if x.dtype != torch.float32:
            x = x.float()
        if x.dim() != 2 or x.stride(1) != 1:
            x = x.contiguous()
        dims = self.dims()
        if x.shape[1] != dims[0]:
            raise ValueError(f"input dim {x.shape[1]} != encoder input dim {dims[0]}")
        B = x.shape[0]
        packed = self.packed_weights()
        if out is not None:   # caller-owned key table (pipelined batches keep theirs across streams)
            keys, nkeys = out
            if keys.shape != (B, n) or keys.dtype != torch.int32 or nkeys.shape != (B,) or nkeys.dtype != torch.int32:
                raise ValueError("out must be (int32 [B, n], int32 [B])")
        else:
            keys = torch.empty((B, n), dtype=torch.int32, device=x.device)
            nkeys = torch.empty((B,), dtype=torch.int32, device=x.device)
        probs = torch.empty((B, self._hash_size), dtype=torch.float32, device=x.device) if want_probs else None
        if ranked:
            seed = 0              # no draw is made: the call counter of the sampled mode's seeds is left alone
        elif seed is None:
            seed = (self._seed + 0x9E3779B97F4A7C15 * (next(self._calls) + 1)) & 0xFFFFFFFFFFFFFFFF
        stream = torch.cuda.current_stream(x.device).cuda_stream
        n_multi = B if n_multi_rows is None else int(n_multi_rows)
        # ranked: the encode makes one probe and hands out z and the hard code; nlsh_probe_ranked then fills the caller's table
        ekeys, enkeys, en = keys, nkeys, n
        ranked = ranked and n > 1     # one probe is the hard key in either mode
        if ranked:
            en = 1
            ekeys = torch.empty((B, 1), dtype=torch.int32, device=x.device)
            enkeys = torch.empty((B,), dtype=torch.int32, device=x.device)
            if z_out is None:
                z_out = torch.empty((B, self._hash_size), dtype=torch.float32, device=x.device)
            if code_out is None:
                code_out = torch.empty((B,), dtype=torch.int32, device=x.device)
        if self.streamed():
            ws = self._stream_workspace(L, dims, B, x.device, stream)
            _capi.check(L.nlsh_encode_hash_stream(
                _capi.ptr(x), B, x.stride(0) if B else dims[0], len(dims) - 1, _capi.int_array(dims), _capi.ptr(packed),
                _capi.ACT_TANH if self._tanh_output else _capi.ACT_SIGMOID, self.key_mode, en, n_multi, seed, row0,
                _capi.ptr(z_out), _capi.ptr(probs), _capi.ptr(code_out), _capi.ptr(ekeys), _capi.ptr(enkeys),
                _capi.ptr(ws), ws.numel(), stream))
        else:
            _capi.check(L.nlsh_encode_hash(
                _capi.ptr(x), B, x.stride(0) if B else dims[0], len(dims) - 1, _capi.int_array(dims), _capi.ptr(packed),
                _capi.ACT_TANH if self._tanh_output else _capi.ACT_SIGMOID, self.key_mode, en, n_multi, seed, row0,
                _capi.ptr(z_out), _capi.ptr(probs), _capi.ptr(code_out), _capi.ptr(ekeys), _capi.ptr(enkeys), stream))
        if ranked:
            _capi.check(L.nlsh_probe_ranked(_capi.ptr(z_out), z_out.stride(0) if B else self._hash_size, _capi.ptr(code_out), B,
                                            self._hash_size, self.key_mode, n, n_multi, _capi.ptr(keys), _capi.ptr(nkeys), None, stream))
        return keys, nkeys, probs


def host_key_set(row, count, key_mode=_capi.KEY_REF_INT16) -> Set[int]:
    """One row of a HOST key table -> the reference's key set (same construction as `keys_to_sets`, so the same
    Python iteration order: the F7 fallback names the LAST key of that order)."""
    if key_mode == _capi.KEY_FULL:
        row = row.astype("int64") & 0xFFFFFFFF
    return set(row[:count].tolist())


def keys_to_sets(keys, nkeys, key_mode=_capi.KEY_REF_INT16) -> List[Set[int]]:
    """Device key table -> the reference's `List[Set[int]]` (one D2H copy, then host objects)."""
    kh = keys.cpu().numpy()
    nh = nkeys.cpu().numpy()
    if key_mode == _capi.KEY_FULL:
        kh = kh.astype("int64") & 0xFFFFFFFF  # eval.py:49-53 yields non-negative ints
    return [set(row[:c].tolist()) for row, c in zip(kh, nh)]


class _CategoricalHasher(nn.Module):
    """encoder -> Linear(hash_size) -> softmax; the reference module's child names (hashings.py:97-107: `_encoder`, `output_layer`),
    so state dicts interchange."""

    def __init__(self, encoder, hash_size):
        super().__init__()
        self._encoder = encoder
        self.output_layer = nn.Linear(encoder.output_dim, hash_size)

    def forward(self, x):  # stock autograd path: training only (out of the hot path)
        return torch.softmax(self.output_layer(self._encoder(x)), dim=1)


class Categorical(_DeviceHashing):
    """The reference's `Categorical` (nlsh/hashings.py:95-139): a softmax over `hash_size` bins, the bucket is the argmax bin.  The
    forward is `nlsh_encode_logits` (the layer GEMMs of the streamed form, any width up to `_capi.MAX_BINS`), the keys come from
    `nlsh_probe_bins`: a row's n most probable bins, best first (softmax is monotone, so the kernel ranks logits).  Keys are bin
    indices (`key_mode = KEY_FULL`); the multi-probe is ranked by construction -- a softmax has no Bernoulli draws.  There is no
    `encode_args` / `ranked_encode_args`: `Indexer` hashes, then scans (`last_query_path == "two_step"`); pipelined batch slots and
    `ShardedIndexer` refuse this family."""
    _Hasher = _CategoricalHasher
    hash_family = "categorical"
    key_mode = _capi.KEY_FULL

    def __init__(self, encoder, hash_size, distance_func, seed=0):
        if not 1 <= hash_size <= _capi.MAX_BINS:
            raise ValueError(f"hash_size must be in [1, {_capi.MAX_BINS}], got {hash_size}")
        self._init_hasher(encoder, hash_size, distance_func, _CategoricalHasher(encoder, hash_size), seed)

    @property
    def probes(self):
        return "ranked"

    @probes.setter
    def probes(self, mode):
        self._ranked_only(mode)

    @staticmethod
    def _ranked_only(mode):
        if _capi.probe_mode(mode, "ranked") != "ranked":
            raise ValueError("Categorical probes are ranked only (the next most probable bins): a softmax has no Bernoulli draws to sample")

    # ------------------------------------------------------------------ reference surface
    def predict(self, x):
        """Softmax probabilities [B, M].  Eval mode: `torch.softmax` of the device logits (plumbing, not the query path).  Train mode:
        the autograd forward."""
        if self._hasher.training:
            return self._hasher(x)
        return torch.softmax(self.logits_device(x), dim=1)

    def hash(self, query_vectors, n=None, probes=None):
        """n=None: the reference's `List[int]`, every row's argmax bin (hashings.py:131-133).  An integer n >= 1: `List[Set[int]]` of the
        n most probable bins, like `MultivariateBernoulli.hash`."""
        self._ranked_only(probes)
        keys, nkeys = self.hash_device(query_vectors, n=1 if n is None else n)
        if n is None:
            return keys[:, 0].tolist()
        return keys_to_sets(keys, nkeys, self.key_mode)

    # ------------------------------------------------------------------ device-resident form
    def logits_device(self, x):
        """-> logits fp32 [B, M]: one layer-GEMM launch per Linear layer, `oracle.mlp_forward`'s arithmetic bit for bit."""
        if x.device.type != "cuda":
            raise _capi.NlshHipError(_capi.E_INVALID, "encode_logits needs a device tensor; there is no CPU path")
        if self._needs_train_forward():
            raise _capi.NlshHipError(_capi.E_UNSUPPORTED, "Categorical needs eval mode for BatchNorm encoders (train_mode(False)): the "
                                                          "device forward folds the running statistics into its weights")
        L = _capi.lib()
        x = x.detach()
        if x.dtype != torch.float32:
            x = x.float()
        if x.dim() != 2 or x.stride(1) != 1:
            x = x.contiguous()
        dims = self.dims()
        if x.shape[1] != dims[0]:
            raise ValueError(f"input dim {x.shape[1]} != encoder input dim {dims[0]}")
        B, M = x.shape[0], dims[-1]
        packed = self.packed_weights()
        logits = torch.empty((B, M), dtype=torch.float32, device=x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        ws = self._stream_workspace(L, dims, B, x.device, stream, L.nlsh_logits_workspace)
        _capi.check(L.nlsh_encode_logits(_capi.ptr(x), B, x.stride(0) if B else dims[0], len(dims) - 1, _capi.int_array(dims), _capi.ptr(packed),
                                         _capi.ptr(logits), M, _capi.ptr(ws), ws.numel(), stream))
        return logits

    def _key_tables(self, B, n, out, device):
        if n < 1:
            raise ValueError(f"`n` should be positive integer, but got {n}")
        if n > _capi.MAX_ENCODE_PROBES:
            raise _capi.NlshHipError(_capi.E_UNSUPPORTED, f"hash_times={n} > {_capi.MAX_ENCODE_PROBES}")
        if out is None:
            return torch.empty((B, n), dtype=torch.int32, device=device), torch.empty((B,), dtype=torch.int32, device=device)
        keys, nkeys = out
        if keys.shape != (B, n) or keys.dtype != torch.int32 or nkeys.shape != (B,) or nkeys.dtype != torch.int32:
            raise ValueError("out must be (int32 [B, n], int32 [B])")
        return keys, nkeys

    def hash_device(self, x, n=1, n_multi_rows=None, seed=None, row0=0, out=None, probes=None):
        """-> (keys int32 [B, n]: the row's min(n, M) best bins, best first, then zeros; nkeys int32 [B]) on the device.  Rows >=
        n_multi_rows are single-probe (Indexer.hash's trailing-batch rule).  The keys are a function of the row alone: `seed` and
        `row0` are accepted and ignored."""
        self._ranked_only(probes)
        B = x.shape[0]
        keys, nkeys = self._key_tables(B, n, out, x.device)
        logits = self.logits_device(x)
        _capi.check(_capi.lib().nlsh_probe_bins(_capi.ptr(logits), logits.stride(0) if B else self._hash_size, B, self._hash_size, n,
                                                B if n_multi_rows is None else int(n_multi_rows), _capi.ptr(keys), _capi.ptr(nkeys), None,
                                                torch.cuda.current_stream(x.device).cuda_stream))
        return keys, nkeys

    def hash_budget_device(self, x, n, n_multi_rows, uniq_keys, offsets, n_buckets, budget, out=None):
        """`hash_device` cut at a candidate budget on an index's CSR arrays (`nlsh_probe_bins_budget`; n is the cap) ->
        (keys, nkeys, ncand int32 [B])."""
        B = x.shape[0]
        keys, nkeys = self._key_tables(B, n, out, x.device)
        ncand = torch.empty((B,), dtype=torch.int32, device=x.device)
        logits = self.logits_device(x)
        _capi.check(_capi.lib().nlsh_probe_bins_budget(
            _capi.ptr(logits), logits.stride(0) if B else self._hash_size, B, self._hash_size, n, B if n_multi_rows is None else int(n_multi_rows),
            _capi.ptr(uniq_keys), _capi.ptr(offsets), int(n_buckets), int(budget), _capi.ptr(keys), _capi.ptr(nkeys), None, _capi.ptr(ncand),
            torch.cuda.current_stream(x.device).cuda_stream))
        return keys, nkeys, ncand

    # ------------------------------------------------------------------ internals
    def _pack_calls(self, L):
        return L.nlsh_logits_packed_floats, L.nlsh_logits_pack
