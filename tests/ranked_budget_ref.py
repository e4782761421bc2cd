"""Pure-Python reference of `nlsh_probe_ranked_budget` (include/nlsh_hip.h): the definition evaluated literally -- the unbudgeted table
of tests/ranked_ref.py, every key's bucket size by `np.searchsorted` on `uniq_keys`, then the prefix cut at the first key that brings the
row's candidate count to the budget."""
import numpy as np

import ranked_ref as rr

INT32_MAX = 2 ** 31 - 1


def sizes_of(keys, uniq_keys, offsets):
    """size(key) of every entry of an int32 array: offsets[b+1] - offsets[b] where uniq_keys[b] == key, else 0."""
    keys = np.asarray(keys, dtype=np.int32)
    uniq_keys = np.asarray(uniq_keys, dtype=np.int32)
    if len(uniq_keys) == 0:
        return np.zeros(keys.shape, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    b = np.minimum(np.searchsorted(uniq_keys, keys), len(uniq_keys) - 1)
    return np.where(uniq_keys[b] == keys, offsets[b + 1] - offsets[b], 0)


def cut(keys, nkeys, cost, uniq_keys, offsets, budget):
    """The prefix cut of an unbudgeted table (`rr.table`'s outputs) -> (keys, nkeys, cost bits, ncand) of the budgeted call."""
    n, P = keys.shape
    out_keys, out_cost = np.zeros_like(keys), np.full_like(cost, rr.INF_BITS)
    out_nkeys, ncand = np.zeros_like(nkeys), np.zeros((n,), dtype=np.int32)
    for r in range(n):
        nk = int(nkeys[r])
        cum = np.cumsum(sizes_of(keys[r, :nk], uniq_keys, offsets))          # cum[m - 1] = cum(m)
        reached = np.nonzero(cum >= budget)[0]
        m = int(reached[0]) + 1 if len(reached) else nk
        out_keys[r, :m], out_cost[r, :m], out_nkeys[r], ncand[r] = keys[r, :m], cost[r, :m], m, cum[m - 1]
    return out_keys, out_nkeys, out_cost, ncand


def table(z, codes, H, P, key_mode, uniq_keys, offsets, budget, n_multi_rows=None, fn=rr.best_first):
    """Expected outputs of one `nlsh_probe_ranked_budget` call: (keys int32 [n, P] zero padded, nkeys int32 [n], cost bits uint32
    [n, P] with +inf past nkeys, ncand int32 [n])."""
    return cut(*rr.table(z, codes, H, P, key_mode, n_multi_rows=n_multi_rows, fn=fn), uniq_keys, offsets, budget)


def unbudgeted_cum(keys, nkeys, uniq_keys, offsets):
    """cum(nk) of every row of an unbudgeted table: the candidates the row has without a budget."""
    valid = np.arange(keys.shape[1])[None, :] < nkeys[:, None]
    return (sizes_of(keys, uniq_keys, offsets) * valid).sum(1)


def median_budget(keys, nkeys, uniq_keys, offsets):
    """The tests' middle budget: the median over rows of the unbudgeted cum(nk) / 2, at least 1."""
    return max(1, int(np.median(unbudgeted_cum(keys, nkeys, uniq_keys, offsets) / 2)))


def heavy_tailed_csr(uniq_keys, seed):
    """offsets for ascending `uniq_keys`: bucket sizes with many 1s, some zero-length buckets and a few in the thousands."""
    rng = np.random.default_rng(seed)
    nb = len(uniq_keys)
    u = rng.random(nb)
    sizes = np.where(u < 0.1, 0, np.where(u < 0.7, 1, np.where(u < 0.97, rng.integers(2, 40, size=nb), rng.integers(1000, 5000, size=nb))))
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def sampled_uniq_keys(nb, H, key_mode, seed, include=()):
    """`nb` distinct keys of the code space of an H-bit hash, ascending as signed int32 (`include`: keys that must be among them)."""
    rng = np.random.default_rng(seed)
    bits = min(H, 16) if key_mode == rr.KEY_REF_INT16 else H
    nb = min(nb, 1 << bits)
    if (1 << bits) <= 4 * nb + 1024:
        codes = rng.permutation(1 << bits)[:nb].astype(np.int64)
    else:
        codes = np.unique(rng.integers(0, 1 << bits, size=2 * nb + 64, dtype=np.int64))
        codes = rng.permutation(codes)[:nb]
    keys = {rr.key_of(int(c), key_mode) for c in codes}
    missing = {int(key) for key in include} - keys
    spare = rng.permutation(sorted(keys - {int(key) for key in include})).tolist()
    keys = (keys - set(spare[:len(missing)])) | missing           # the count stays nb where there are keys to give up
    return np.array(sorted(keys), dtype=np.int32)
