"""Numpy reference of `nlsh_probe_bins` / `nlsh_probe_bins_budget` (include/nlsh_hip.h): the definition written twice -- a stable sort on
(u(z) descending, bin ascending) and a repeated-argmax loop -- plus the budget rule as a walk and as a prefix-sum cut, and the row
generators the CPU and GPU tests share."""
import numpy as np

import ranked_budget_ref as rbr

INT32_MAX = rbr.INT32_MAX
NEG_INF_BITS = 0xFF800000


def order_bits(z):
    """u(z): the IEEE total-order map of float32 bit patterns to uint32 (negative: complemented; non-negative: sign bit set)."""
    b = np.ascontiguousarray(z, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def ranked_by_sort(row, n):
    """The first min(n, M) bins of one row by a stable sort: descending u, ties in ascending bin order."""
    u = order_bits(row).astype(np.int64)
    return np.argsort(-u, kind="stable")[:min(n, len(row))].tolist()


def ranked_by_argmax(row, n):
    """The same bins by n rounds of 'the best bin not taken yet' (np.argmax names the first of equal maxima: the smallest bin)."""
    u = order_bits(row).astype(np.int64)
    out = []
    for _ in range(min(n, len(row))):
        b = int(np.argmax(u))
        out.append(b)
        u[b] = -1
    return out


def table(logits, n_probes, n_multi_rows=None, fn=ranked_by_sort):
    """Expected outputs of one `nlsh_probe_bins` call: (keys int32 [n, P] zero padded, nkeys int32 [n], logit bits uint32 [n, P] with
    -inf past nkeys)."""
    logits = np.asarray(logits, dtype=np.float32)
    n = logits.shape[0]
    multi = n if n_multi_rows is None else n_multi_rows
    keys = np.zeros((n, n_probes), dtype=np.int32)
    nkeys = np.zeros((n,), dtype=np.int32)
    bits = np.full((n, n_probes), NEG_INF_BITS, dtype=np.uint32)
    for r in range(n):
        bins = fn(logits[r], n_probes if r < multi else 1)
        keys[r, :len(bins)], nkeys[r] = bins, len(bins)
        bits[r, :len(bins)] = logits[r, bins].view(np.uint32)
    return keys, nkeys, bits


def cut(keys, nkeys, bits, uniq_keys, offsets, budget):
    """The budget rule as a prefix-sum cut of an unbudgeted table -> (keys, nkeys, logit bits, ncand)."""
    n = keys.shape[0]
    out_keys, out_bits = np.zeros_like(keys), np.full_like(bits, NEG_INF_BITS)
    out_nkeys, ncand = np.zeros_like(nkeys), np.zeros((n,), dtype=np.int32)
    for r in range(n):
        nk = int(nkeys[r])
        cum = np.cumsum(rbr.sizes_of(keys[r, :nk], uniq_keys, offsets))
        reached = np.nonzero(cum >= budget)[0]
        m = int(reached[0]) + 1 if len(reached) else nk
        out_keys[r, :m], out_bits[r, :m], out_nkeys[r], ncand[r] = keys[r, :m], bits[r, :m], m, cum[m - 1]
    return out_keys, out_nkeys, out_bits, ncand


def walk(keys, nkeys, bits, uniq_keys, offsets, budget):
    """The budget rule word for word: walk the keys, keep through the first one that brings the candidates to the budget."""
    size_of = {int(k): int(offsets[b + 1] - offsets[b]) for b, k in enumerate(uniq_keys)}
    n = keys.shape[0]
    out_keys, out_bits = np.zeros_like(keys), np.full_like(bits, NEG_INF_BITS)
    out_nkeys, ncand = np.zeros_like(nkeys), np.zeros((n,), dtype=np.int32)
    for r in range(n):
        kept, cum = 0, 0
        for s in range(int(nkeys[r])):
            kept, cum = kept + 1, cum + size_of.get(int(keys[r, s]), 0)
            if cum >= budget:
                break
        out_keys[r, :kept], out_bits[r, :kept], out_nkeys[r], ncand[r] = keys[r, :kept], bits[r, :kept], kept, cum
    return out_keys, out_nkeys, out_bits, ncand


# ------------------------------------------------------------------------------------------------ rows
def random_rows(n, M, seed):
    return np.random.default_rng(seed).standard_normal((n, M)).astype(np.float32)


def tie_rows(n, M, seed):
    """Mass ties: every logit is one of three values."""
    return np.random.default_rng(seed).choice(np.array([-1.5, 0.25, 2.0], dtype=np.float32), size=(n, M))


def equal_rows(n, M, value=0.75):
    return np.full((n, M), value, dtype=np.float32)


def special_rows(n, M, seed):
    """+-inf, -0 / +0 and ordinary values mixed, each with several copies per row."""
    rng = np.random.default_rng(seed)
    pool = np.array([np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 3.0e38, -3.0e38, 1e-45, -1e-45], dtype=np.float32)
    z = pool[rng.integers(0, len(pool), size=(n, M))]
    z[::3] = np.where(rng.random((len(z[::3]), M)) < 0.5, np.float32(0.0), np.float32(-0.0))     # rows of zeros of both signs only
    return z


def mixed_rows(n, M, seed):
    z = random_rows(n, M, seed)
    z[1::4] = tie_rows(len(z[1::4]), M, seed + 1)
    z[2::4] = special_rows(len(z[2::4]), M, seed + 2)
    z[3::4] = equal_rows(len(z[3::4]), M)
    return z


def bin_csr(M, seed, present=0.6):
    """CSR arrays over bin keys: a random `present` share of the M bins has a bucket (so some probed bins have none), heavy-tailed sizes."""
    rng = np.random.default_rng(seed)
    uniq = np.nonzero(rng.random(M) < present)[0].astype(np.int32)
    if len(uniq) == 0:
        uniq = np.array([M - 1], dtype=np.int32)
    return uniq, rbr.heavy_tailed_csr(uniq, seed + 1)
