"""Pure-Python reference of `nlsh_probe_ranked` (include/nlsh_hip.h), numpy float32 arithmetic: the definition evaluated literally
(`brute`: all 2^H subsets, sorted) and the best-first search the kernel runs (`best_first`: a heap), which the CPU tests hold against
each other so that the GPU tests can use the heap form at hash sizes `brute` cannot enumerate."""
import heapq

import numpy as np

KEY_REF_INT16, KEY_FULL = 0, 1
INF_BITS = 0x7F800000


def sorted_costs(z_row, H):
    """(c fp32 [H] in sorted order, s: bit index at each sorted position): step 1 of the definition."""
    bits = np.ascontiguousarray(np.asarray(z_row, dtype=np.float32)[:H]).view(np.uint32) & np.uint32(0x7FFFFFFF)
    s = sorted(range(H), key=lambda h: (int(bits[h]), h))
    return bits[s].astype(np.uint32).view(np.float32), s


def key_of(code, key_mode):
    """The bucket key of a code as the signed int32 the key table holds."""
    code &= 0xFFFFFFFF
    if key_mode == KEY_REF_INT16:
        code &= 0xFFFF
        return code - (1 << 16) if code >= (1 << 15) else code
    return code - (1 << 32) if code >= (1 << 31) else code


def _finish(subsets, code, H, s, key_mode):
    """[(cost bits, mask)] in order -> (keys, cost bits) of the slots kept by the first-occurrence de-duplication."""
    keys, costs = [], []
    for bits, mask in subsets:
        flip = 0
        for i in range(H):
            if (mask >> i) & 1:
                flip |= 1 << (H - 1 - s[i])
        key = key_of(int(code) ^ flip, key_mode)
        if key not in keys:
            keys.append(key)
            costs.append(bits)
    return keys, costs


def brute(z_row, code, H, P, key_mode):
    """The definition, literally: every mask's chain (vectorised over the masks: position i ascending, t = t + c[s[i]] where bit i
    is set), sorted by (cost bit pattern, mask), the first min(P, 2^H)."""
    c, s = sorted_costs(z_row, H)
    masks = np.arange(1 << H, dtype=np.uint64)
    t = np.zeros(1 << H, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(H):
            t = np.where((masks >> np.uint64(i)) & np.uint64(1), t + c[i], t).astype(np.float32)
    bits = t.view(np.uint32)
    order = sorted(range(1 << H), key=lambda m: (int(bits[m]), m))[:P]
    return _finish([(int(bits[m]), m) for m in order], code, H, s, key_mode)


def best_first(z_row, code, H, P, key_mode):
    """The shift / expand search: the frontier starts at {0}; a pop pushes the shift child (chain without its last term + the next
    cost) and the expand child (chain + the next cost)."""
    c, s = sorted_costs(z_row, H)
    f32 = np.float32
    out = [(0, 0)]
    with np.errstate(all="ignore"):
        heap = [(int(f32(f32(0.0) + c[0]).view(np.uint32)), 1, f32(0.0))]
        while heap and len(out) < P:
            bits, mask, t_prev = heapq.heappop(heap)
            out.append((bits, mask))
            j = mask.bit_length() - 1
            if j + 1 < H:
                t = np.uint32(bits).view(f32)
                heapq.heappush(heap, (int(f32(t_prev + c[j + 1]).view(np.uint32)), mask ^ (3 << j), t_prev))
                heapq.heappush(heap, (int(f32(t + c[j + 1]).view(np.uint32)), mask | (1 << (j + 1)), t))
    return _finish(out, code, H, s, key_mode)


def table(z, codes, H, P, key_mode, n_multi_rows=None, fn=best_first):
    """Expected outputs of one `nlsh_probe_ranked` call: (keys int32 [n, P] zero padded, nkeys int32 [n], cost bits uint32 [n, P]
    with +inf past nkeys)."""
    n = len(codes)
    n_multi_rows = n if n_multi_rows is None else n_multi_rows
    keys = np.zeros((n, P), dtype=np.int32)
    nkeys = np.zeros((n,), dtype=np.int32)
    cost = np.full((n, P), INF_BITS, dtype=np.uint32)
    for r in range(n):
        k, c = fn(z[r], int(codes[r]) & 0xFFFFFFFF, H, P if r < n_multi_rows else 1, key_mode)
        keys[r, :len(k)], cost[r, :len(k)], nkeys[r] = k, c, len(k)
    return keys, nkeys, cost


# ---------------------------------------------------------------------------- the rows the tests share
def random_rows(n, H, seed):
    return np.random.default_rng(seed).standard_normal((n, H)).astype(np.float32)


def tie_rows(n, H, seed):
    """Mass ties: every value from {0.0, -0.0, +-0.5, +-1.0}."""
    vals = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0], dtype=np.float32)
    return vals[np.random.default_rng(seed).integers(0, len(vals), size=(n, H))]


def absorbing_rows(n, H, seed):
    """Magnitudes from 1e-8 to 1e8 and +-inf: small terms are absorbed by large ones, so different chains round to equal costs."""
    rng = np.random.default_rng(seed)
    mag = (10.0 ** rng.integers(-8, 9, size=(n, H))).astype(np.float32)
    mag[rng.random((n, H)) < 0.15] = np.inf
    return (mag * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(n, H))).astype(np.float32)


def hard_codes(z, H):
    """The hard code a sigmoid / tanh head gives a row of pre-activations: bit h of the hasher (p > 0.5, i.e. z > 0) at code bit H-1-h."""
    codes = np.zeros((z.shape[0],), dtype=np.uint32)
    for h in range(H):
        codes |= (z[:, h] > 0).astype(np.uint32) << np.uint32(H - 1 - h)
    return codes
