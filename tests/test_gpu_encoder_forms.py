"""GPU: every kernel form of `nlsh_encode_hash` across architectures, probe counts and partial last workgroups.
Each call goes straight to the C ABI with outputs of the test's own, 64 sentinel words behind each; before it, `nlsh_encode_form`
must name the intended form.  References are the oracle's forward, head, bit rule, packing and Philox sampler -- never the library.
The last test of the module asserts that all six forms ran."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import encoder_form_cases as fc
from encoder_form_cases import BUILD128, H16, HET, PINGPONG, SINGLE, SINGLE_WIDE
from helpers import dev, make_hashing
from nlsh_amd import _capi, synth
from oracle import oracle

pytestmark = pytest.mark.gpu

EXERCISED = set()            # form ids that were launched (and whose outputs were checked) by this module
GUARD = 64                   # sentinel words behind every output
PATTERN = 0x5A5A5A5A         # as float32 1.5e16: no probability, no z of these encoders, no key of <= 31 bits with this value by chance
ROW0S = (0, 7, 2 ** 32 - 100)            # the last one: the Philox counter's high word changes at row 100 of the batch
PROBES = (1, 10, 64, 65, 128)            # both de-duplication paths (<= 64 | serial), and the probe-sized row stride of narrow encoders
MODES = ((_capi.KEY_REF_INT16, "ref_int16"), (_capi.KEY_FULL, "full"))
ACTS = ((_capi.ACT_SIGMOID, "sigmoid"), (_capi.ACT_TANH, "tanh"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _round_rows():
    return 32 * fc.cus()


class _Encoder:
    """A layer stack on the device, packed for `nlsh_encode_hash` from numpy weights."""

    def __init__(self, dims, Ws, bs):
        L = _capi.lib()
        self.dims, self.Ws, self.bs = list(dims), Ws, bs
        self._w = [dev(W) for W in Ws]
        self._b = [None if b is None else dev(b) for b in bs]
        arr = _capi.int_array(self.dims)
        n_floats = L.nlsh_encoder_packed_floats(len(Ws), arr)
        assert n_floats > 0
        self.packed = torch.empty((n_floats,), dtype=torch.float32, device="cuda")
        _capi.check(L.nlsh_encoder_pack(len(Ws), arr, _capi.ptr_array(self._w), _capi.ptr_array(self._b), _capi.ptr(self.packed),
                                        torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()


def _encode(enc, x, form, n_probes, n_multi, seed, row0, key_mode, act):
    """One guarded `nlsh_encode_hash` call on the rows of `x` (a device tensor, any row stride) -> host arrays."""
    n, H = x.shape[0], enc.dims[-1]
    assert x.dtype == torch.float32 and x.stride(1) == 1
    got = _capi.encode_form(n, enc.dims, n_probes)[0]
    assert got == form, f"{_capi.ENC_FORM_NAMES[got]} selected, {_capi.ENC_FORM_NAMES[form]} intended"
    sizes = dict(z=n * H, p=n * H, code=n, keys=n * n_probes, nkeys=n)
    bufs = {k: torch.full((v + GUARD,), PATTERN, dtype=torch.int32, device="cuda") for k, v in sizes.items()}
    _capi.check(_capi.lib().nlsh_encode_hash(
        _capi.ptr(x), n, x.stride(0), len(enc.dims) - 1, _capi.int_array(enc.dims), _capi.ptr(enc.packed), act, key_mode, n_probes,
        n_multi, seed, row0, _capi.ptr(bufs["z"]), _capi.ptr(bufs["p"]), _capi.ptr(bufs["code"]), _capi.ptr(bufs["keys"]),
        _capi.ptr(bufs["nkeys"]), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    EXERCISED.add(form)
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, v in sizes.items():
        assert np.all(host[k][v:] == PATTERN), f"{k}: a store behind the end of the output"
    return dict(z=host["z"][:sizes["z"]].view(np.float32).reshape(n, H), p=host["p"][:sizes["p"]].view(np.float32).reshape(n, H),
                code=host["code"][:n].view(np.uint32), keys=host["keys"][:sizes["keys"]].reshape(n, n_probes), nkeys=host["nkeys"][:n])


def _p01(p, act_name):
    """Bernoulli probability of the module output, in fp32 as hashings.py:68-69 forms it."""
    return (p / np.float32(2.0) + np.float32(0.5)).astype(np.float32) if act_name == "tanh" else p


def _check_epilogue(out, n_probes, n_multi, seed, row0, mode, act_name):
    """code, keys and key counts against the oracle's bit rule, packing and sampler applied to the DEVICE's probabilities."""
    n = out["p"].shape[0]
    p01 = _p01(out["p"], act_name)
    code_o = oracle.pack_keys(oracle.hard_bits(p01)[:, None, :], "full")[:, 0]
    assert np.array_equal(out["code"].astype(np.int64), code_o), "hard code"
    ko, no = oracle.row_keys(p01, n_probes, mode, seed=seed, n_multi_rows=n_multi, row0=row0)
    assert np.array_equal(out["nkeys"], no), f"nkeys differ on {int((out['nkeys'] != no).sum())} rows"
    assert np.all(out["nkeys"][n_multi:] == 1), "a row at or past n_multi_rows has more than one key"
    kd = out["keys"].astype(np.int64)
    if mode == "full":
        kd &= 0xFFFFFFFF
    live = np.arange(n_probes)[None, :] < no[:, None]
    assert np.array_equal(kd[live], ko[live]), "live keys"
    return no


def _check_all(out, zo, n_probes, n_multi, seed, row0, mode, act_name):
    assert np.array_equal(_bits(out["z"]), _bits(zo)), f"z not bit-exact: {int((_bits(out['z']) != _bits(zo)).sum())} words, max |dz| {np.abs(out['z'] - zo).max()}"
    raw_o, _ = oracle.head_probs(zo, act_name)
    err = float(np.abs(out["p"] - raw_o).max())
    assert err <= 2e-7, f"probs off by {err}"          # the project's bound: device expf / tanhf vs glibc, 1-2 ulp of a value in (0, 1)
    return _check_epilogue(out, n_probes, n_multi, seed, row0, mode, act_name)


def _forward(x, Ws, bs):
    """oracle.mlp_forward over row chunks on a few threads (rows are independent; the C call releases the GIL)."""
    n = x.shape[0]
    cuts = np.linspace(0, n, max(1, min(8, n // 256)) + 1).astype(int)
    with ThreadPoolExecutor(8) as ex:
        parts = list(ex.map(lambda i: oracle.mlp_forward(x[cuts[i]:cuts[i + 1]], Ws, bs), range(len(cuts) - 1)))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def _reference(dims):
    """(encoder, x on the device, the oracle's z) of an architecture at the most rows the grid runs it at: computed once, read-only,
    every case of the architecture takes its leading rows."""
    dims = list(dims)
    n = fc.max_rows(dims, _round_rows())
    Ws, bs = synth.make_weights(dims, seed=7, gain=3.0)     # |z| around 1: decided and undecided bits, repeated and distinct probes
    x = synth.glove_like(n, dims[0], seed=9)
    zo = _forward(x, Ws, bs)
    zo.setflags(write=False)
    return _Encoder(dims, Ws, bs), dev(x), zo


def _mid_of_a_workgroup(form, n, R):
    """An n_multi_rows that ends in the middle of a workgroup of the form (HET: of a 16-row tail workgroup when the tail has one)."""
    if form == HET:
        rem = n % R
        return n - rem + 21 if rem > 21 else 3 * 32 + 13
    rows = {H16: 16, SINGLE: 32, SINGLE_WIDE: 32, BUILD128: 128, PINGPONG: 64}[form]
    return max(n // 2 // rows, 100 // rows) * rows + rows // 2 + 1      # around n / 2, and past row 100 (where ROW0S[2] carries)


# ----------------------------------------------------------------------------- 1. every output of every form against the oracle
# (index into (0, mid-workgroup, n) for n_multi_rows, index into ROW0S) of the five calls of a case, one per entry of PROBES.  Three
# schedules, taken in turn by consecutive cases.  In each, every n_multi_rows and every row0 occurs, and the row0 whose counter
# carries into the high word meets a multi-probe call with multi-probe rows twice; over the three it does so at every probe count > 1.
SCHEDULES = (
    ((2, 0), (1, 2), (2, 1), (0, 0), (2, 2)),
    ((1, 1), (2, 0), (1, 2), (2, 2), (0, 1)),
    ((2, 1), (2, 2), (0, 0), (1, 2), (1, 0)),
)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_form_outputs_match_oracle(case):
    """Five calls per (form, architecture, n), one per probe count; n_multi_rows (0 | mid-workgroup | n) and row0 follow SCHEDULES,
    key mode and activation rotate with the call and the case: every case sees every value of every axis, the grid sees the pairs."""
    form, dims, nspec = case
    R = _round_rows()
    n = fc.rows(nspec, R)
    enc, xd, zo = _reference(tuple(dims))
    shift = fc.CASES.index(case)
    multi = (0, _mid_of_a_workgroup(form, n, R), n)
    assert 100 < multi[1] < n                   # (the high word of the Philox counter changes at row 100: inside the multi-probe rows)
    counts = []
    for i, n_probes in enumerate(PROBES):
        n_multi, row0 = multi[SCHEDULES[shift % 3][i][0]], ROW0S[SCHEDULES[shift % 3][i][1]]
        (key_mode, mode), (act, act_name) = MODES[(i + shift) % 2], ACTS[((i + shift) // 2) % 2]
        seed = (0x9E3779B97F4A7C15 * (shift + 1) + i) & 0xFFFFFFFFFFFFFFFF
        out = _encode(enc, xd[:n], form, n_probes, n_multi, seed, row0, key_mode, act)
        no = _check_all(out, zo[:n], n_probes, n_multi, seed, row0, mode, act_name)
        counts.append((n_probes, n_multi, int(no.max())))
    # the sampler was not idle: some multi-probe call of the case produced more than one key on some row
    assert any(c > 1 for p, m, c in counts if p > 1 and m > 0), counts


# ----------------------------------------------------------------------------- 2. saturated and undecided bits
SATURATED = {   # form -> (hidden part of the architecture, n)
    H16: ([50, 64, 64], 4095), SINGLE: ([25, 96], 4097), HET: ([25, 96], "R+1"), SINGLE_WIDE: ([64, 257], 130),
    BUILD128: ([25, 96], 16385), PINGPONG: ([100, 300], 16385),
}


def _constant_head(form, bias):
    """Encoder of the form's architecture whose output layer is W = 0 with the given bias: every product of the output chain is a
    zero, the chain sums to +0.0, so z = +0.0 + bias for any finite input -- the bias itself (-0.0 arrives as +0.0)."""
    hidden, nspec = SATURATED[form]
    n = fc.rows(nspec, _round_rows())
    bias = np.asarray(bias, dtype=np.float32)
    dims = hidden + [len(bias)]
    Ws, bs = synth.make_weights(dims, seed=31)
    Ws[-1] = np.zeros_like(Ws[-1])
    bs[-1] = bias
    x = dev(synth.glove_like(n, dims[0], seed=13))
    return _Encoder(dims, Ws, bs), x, n, np.broadcast_to(np.float32(0.0) + bias, (n, len(bias)))


@pytest.mark.parametrize("form", sorted(SATURATED), ids=lambda f: _capi.ENC_FORM_NAMES[f])
def test_saturated_and_undecided_bits(form):
    bias = [0.0, -0.0, 30.0, -30.0, 120.0, -120.0] * 2
    enc, x, n, zo = _constant_head(form, bias)
    zero, one, big, neg = [0, 1, 6, 7], [2, 4, 8, 10], [4, 10], [5, 11]
    bits = np.array([0, 0, 1, 0, 1, 0] * 2)
    code = int("".join(map(str, bits)), 2)
    for (act, act_name), (key_mode, mode) in zip(ACTS, MODES):
        out = _encode(enc, x, form, 10, n, 77, 7, key_mode, act)
        _check_all(out, zo, 10, n, 77, 7, mode, act_name)
        p01 = _p01(out["p"], act_name)
        assert np.all(p01[:, zero] == 0.5) and np.all(p01[:, one] == 1.0) and np.all(p01[:, neg] == 0.0)
        if act_name == "tanh":
            assert np.all(out["p"][:, zero] == 0.0) and np.all(out["p"][:, big] == 1.0) and np.all(out["p"][:, neg] == -1.0)
        assert np.all(out["code"] == code)              # both zeros give bit 0 (the rule is strict), +30 / +120 bit 1, -30 / -120 bit 0


@pytest.mark.parametrize("form", sorted(SATURATED), ids=lambda f: _capi.ENC_FORM_NAMES[f])
def test_certain_bits_collapse_every_probe_to_one_key(form):
    """Only +-120: every probability is exactly 0 or 1, every draw repeats the hard code -- the first-occurrence mask keeps one bit."""
    sign = np.random.default_rng(5).integers(0, 2, size=16) * 2 - 1
    enc, x, n, zo = _constant_head(form, 120.0 * sign)
    code = int("".join("1" if s > 0 else "0" for s in sign), 2)
    for n_probes, (key_mode, mode), (act, act_name) in ((64, MODES[1], ACTS[0]), (128, MODES[0], ACTS[1])):
        out = _encode(enc, x, form, n_probes, n, 5, ROW0S[2], key_mode, act)
        _check_all(out, zo, n_probes, n, 5, ROW0S[2], mode, act_name)
        assert np.all(out["nkeys"] == 1) and np.all(out["code"] == code)
        want = code if mode == "full" else int(np.int16(np.uint16(code & 0xFFFF)))
        assert np.all(out["keys"][:, 0].astype(np.int64) & (0xFFFFFFFF if mode == "full" else -1) == want)


@pytest.mark.parametrize("form", sorted(SATURATED), ids=lambda f: _capi.ENC_FORM_NAMES[f])
def test_undecided_bits_fill_the_key_table(form):
    """32 zeros, full keys: every probe is 32 fair draws, so nothing collapses -- rows reach nkeys == n_probes, the mask's other end."""
    enc, x, n, zo = _constant_head(form, [0.0, -0.0] * 16)
    half = np.full((256, 32), 0.5, dtype=np.float32)
    for n_probes in (64, 128):
        _, no = oracle.row_keys(half, n_probes, "full", seed=11, row0=7)      # beforehand, on the oracle alone (the first rows are enough)
        assert int(no.max()) == n_probes
        out = _encode(enc, x, form, n_probes, n, 11, 7, _capi.KEY_FULL, _capi.ACT_SIGMOID)
        assert np.all(out["p"] == 0.5) and np.all(out["code"] == 0)
        counts = _check_all(out, zo, n_probes, n, 11, 7, "full", "sigmoid")
        assert int(counts.max()) == n_probes and int(out["nkeys"].max()) == n_probes


# ----------------------------------------------------------------------------- 3. strided, misaligned input
STRIDED = {   # form -> (architecture with d % 4 != 0, n)
    H16: ([50, 64, 64, 12], 4095), SINGLE: ([25, 96, 8], 4097), HET: ([25, 96, 8], "R+1"), SINGLE_WIDE: ([30, 320, 8], 130),
    BUILD128: ([25, 96, 8], 16385), PINGPONG: ([99, 300, 16], 16385),
}


@pytest.mark.parametrize("form", sorted(STRIDED), ids=lambda f: _capi.ENC_FORM_NAMES[f])
def test_strided_misaligned_input_equals_contiguous(form):
    dims, nspec = STRIDED[form]
    n, d = fc.rows(nspec, _round_rows()), dims[0]
    assert d % 4 != 0
    Ws, bs = synth.make_weights(dims, seed=3)
    enc = _Encoder(dims, Ws, bs)
    wide = dev(synth.glove_like(n, d + 3, seed=4))
    view = wide[:, 1:d + 1]                      # row stride d + 3, first element one float past a 16-byte boundary
    assert view.stride(0) == d + 3 and view.data_ptr() % 16 == 4
    args = (form, 10, _mid_of_a_workgroup(form, n, _round_rows()), 21, 7, _capi.KEY_FULL, _capi.ACT_SIGMOID)
    a, b = _encode(enc, view, *args), _encode(enc, view.contiguous(), *args)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert a["nkeys"].max() > 1


# ----------------------------------------------------------------------------- 4. the fused bucket lookup behind the other forms
@functools.lru_cache(maxsize=None)
def _lookup_data(metric):
    """(query generator, corpus on the device): N = 20000, d = 32; the L2 rows standardised, so that an 11-bit encoder of these
    weights spreads either corpus over more than 256 buckets."""
    if metric == "l2":
        corpus, mean, std = synth.standardise(synth.sift_like(20000, 32, seed=61))
        return (lambda n, seed: synth.standardise(synth.sift_like(n, 32, seed=seed), mean, std)[0]), dev(corpus)
    return (lambda n, seed: synth.glove_like(n, 32, seed=seed)), dev(synth.glove_like(20000, 32, seed=61))


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("hidden,Q,form", [((512,), 100, SINGLE_WIDE), ((512,), 4097, SINGLE_WIDE), ((64, 64), 16385, BUILD128),
                                           ((300,), 16385, PINGPONG)], ids=["wide-100", "wide-4097", "build128", "pingpong"])
def test_one_call_batch_equals_hash_then_scan_behind_every_form(hidden, Q, form, metric):
    """`_batch_tensors` (nlsh_query_batch: the bucket lookup in the encode's epilogue) against `hash_device` + `scan_tensors`: key
    table, key counts, ids, distance bits, candidate counts and 64-bit sort keys, on an index with fewer than 256 buckets and on one
    with more, at P = 1, 10 and 64."""
    from nlsh_amd.data import Glove, SIFT
    from nlsh_amd.indexer import Indexer
    gen, corpus = _lookup_data(metric)
    d, k = 32, 10
    q = dev(gen(Q, 70 + Q))
    for H, compat in ((3, True), (11, False)):
        dims = [d] + list(hidden) + [H]
        Ws, bs = synth.make_weights(dims, seed=61, gain=3.0)
        hashing = make_hashing(d, hidden, H, Ws, bs, compat=compat)
        indexer = Indexer(hashing, corpus, SIFT.distance if metric == "l2" else Glove.distance, compat=compat)
        assert (indexer.n_buckets < 256) == (H == 3), indexer.n_buckets
        for P in (1, 10, 64):
            assert _capi.encode_form(Q, dims, P)[0] == form
            keys, nkeys = indexer.hash_device(q, hash_times=P, seed=4000 + Q)
            want = indexer.scan_tensors(q, keys, nkeys, k=k, want_keys=True)
            got = indexer._batch_tensors(q, k, P, 4000 + Q, want_keys=True)
            assert indexer._fuses(q, P, indexer.last_algo) and indexer.last_query_path == "fused"
            assert torch.equal(got[4], keys) and torch.equal(got[5], nkeys), (H, P)
            for a, w in zip(got[:4], want):
                assert torch.equal(a, w), (H, P)
            EXERCISED.add(form)


# ----------------------------------------------------------------------------- module end
def test_all_six_forms_were_exercised():
    """Runs last in the module: the tests above launched every kernel form (a run of the whole module is what this checks)."""
    missing = [_capi.ENC_FORM_NAMES[f] for f in sorted(fc.ALL_FORMS - EXERCISED)]
    assert not missing, f"forms never launched: {missing}"
