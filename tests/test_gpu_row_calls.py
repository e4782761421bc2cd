"""The row kernels behind `nlsh_gather_rows_typed / _sq8` and `nlsh_csr_update_typed / _sq8`, through the C ABI, on the shapes the storage
tests leave out: every source storage into every destination (float32, float16, uint8, sq8), d = 1, 17, 260 and 1024 (a float16 or
float32 destination row of more than 64 16-byte units wraps the lanes of the update), the source of every gather and the new rows of
every update once on a chunk boundary and once offset by one element with an odd row stride (the element-load path), an index of 0 or
5 rows (two of them removed) taking 0 or 37 new ones.  Everything is compared bit for bit:
  * a gather stores what the storage's rule gives in numpy / torch (`.to(dtype)` of exact values, the sq8 encode formula), zero padded,
    from either source layout;
  * an update gives the arrays of the gather-built rebuild of the same rows (rows, gid, inv_norm, uniq, offsets, src);
  * inv_norm is `nlsh_gather_rows` on the dequantised rows at the float32 default pitch;
  * first_bad names the smallest planted row a storage cannot take, clamped_rows counts every planted saturated row once and not the
    refused one."""
import numpy as np
import pytest
import torch

from nlsh_amd import _capi

pytestmark = pytest.mark.gpu

F32, F16, U8 = _capi.STORE_F32, _capi.STORE_F16, _capi.STORE_U8
CODE = {"float32": F32, "float16": F16, "uint8": U8, "sq8": U8}
TORCH = {"float32": torch.float32, "float16": torch.float16, "uint8": torch.uint8, "sq8": torch.uint8}
PER16 = {"float32": 4, "float16": 8, "uint8": 16, "sq8": 16}
SOURCES, DESTINATIONS = ("float32", "float16", "uint8"), ("float32", "float16", "uint8", "sq8")
DIMS = (1, 17, 260, 1024)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raw(t):
    return t.contiguous().view(torch.uint8).cpu()


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_raw(a), _raw(b)), what


def pitch(dst, d):
    return (d + PER16[dst] - 1) // PER16[dst] * PER16[dst]


def laid_out(values, storage, layout):
    """float32 values [M, d] (exact in `storage`) as a device view [M, d] of that storage: "aligned" = every row on a 16-byte boundary,
    "offset" = one element behind one, rows an odd number of elements apart."""
    M, d = values.shape
    if M == 0:
        return None
    if layout == "aligned":
        wide = torch.zeros((M, (d + 15) // 16 * 16), dtype=TORCH[storage], device="cuda")
        view = wide[:, :d]
    else:
        wide = torch.zeros((M, (d + 2) | 1), dtype=TORCH[storage], device="cuda")
        view = wide[:, 1:d + 1]
    view.copy_(dev(values).to(TORCH[storage]))
    return view


def quantiser(dst, d, rng):
    """sq8: (lo, step) padded to the pitch (lo = 0, step = 1 behind d) under which integers in [0, 255] never saturate."""
    if dst != "sq8":
        return None
    lo, step = np.zeros(pitch(dst, d), np.float32), np.ones(pitch(dst, d), np.float32)
    lo[:d], step[:d] = rng.uniform(-8, 0, d), rng.uniform(1.1, 1.6, d)
    return dev(lo), dev(step)


def csr(keys):
    """keys [n] -> (perm, uniq, offsets) of the stable sort, as nlsh_build_csr gives them."""
    perm = np.argsort(keys, kind="stable").astype(np.int32)
    uniq, first = np.unique(keys[perm], return_index=True)
    return perm, uniq.astype(np.int32), np.append(first, len(keys)).astype(np.int32)


def gather(rows, src, dst, d, perm, quant):
    """`nlsh_gather_rows_typed` / `_sq8` -> (sorted, inv_norm, gid, first_bad, clamped_rows)."""
    L, n, stride = _capi.lib(), len(perm), pitch(dst, d)
    out = torch.full((n, stride), 7, dtype=TORCH[dst], device="cuda")
    inv, gid = torch.empty((n,), dtype=torch.float32, device="cuda"), torch.empty((n,), dtype=torch.int32, device="cuda")
    flags = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    head = (_capi.ptr(rows), CODE[src], rows.stride(0) if n else d, d, _capi.ptr(dev(perm)), n, _capi.ptr(out))
    if dst == "sq8":
        _capi.check(L.nlsh_gather_rows_sq8(*head, stride, _capi.ptr(quant[0]), _capi.ptr(quant[1]), _capi.ptr(inv), _capi.ptr(gid), 0,
                                           _capi.ptr(flags[0:1]), _capi.ptr(flags[1:2]), _stream()))
    else:
        flags[1] = 0
        _capi.check(L.nlsh_gather_rows_typed(*head, CODE[dst], stride, _capi.ptr(inv), _capi.ptr(gid), 0, _capi.ptr(flags[0:1]), _stream()))
    bad, clamped = flags.cpu().tolist()
    return out, inv, gid, bad, clamped


def update(old, uniq_old, offs_old, keep, rows, src, dst, d, keys_new, ids_new, quant):
    """`nlsh_csr_update_typed` / `_sq8` on the gather-built index `old` -> (sorted, inv_norm, gid, src, uniq, offsets, first_bad, clamped)."""
    L, stride = _capi.lib(), pitch(dst, d)
    n_old, m_new, nb_old = len(keep), len(keys_new), len(uniq_old)
    n_kept = int(keep.sum())
    n_out = n_kept + m_new
    out = torch.full((n_out, stride), 7, dtype=TORCH[dst], device="cuda")
    inv, gid = torch.empty((n_out,), dtype=torch.float32, device="cuda"), torch.empty((n_out,), dtype=torch.int32, device="cuda")
    src_out, uniq = torch.empty((n_out,), dtype=torch.int32, device="cuda"), torch.empty((max(n_out, 1),), dtype=torch.int32, device="cuda")
    offs, nb = torch.empty((n_out + 1,), dtype=torch.int32, device="cuda"), torch.full((1,), -5, dtype=torch.int32, device="cuda")
    flags = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    wb = L.nlsh_csr_update_workspace(n_old, nb_old, m_new)
    assert wb > 0
    ws = torch.empty((wb,), dtype=torch.uint8, device="cuda")
    held = (dev(uniq_old), dev(offs_old), dev(keep.astype(np.uint8)), dev(keys_new), dev(ids_new))      # alive across the call
    p = lambda t, n: _capi.ptr(t) if n else None      # noqa: E731
    index = (stride, d, p(old[2], n_old), p(old[1], n_old), p(held[0], n_old), p(held[1], n_old), n_old, nb_old, p(held[2], n_old), n_kept)
    new = (rows.stride(0) if m_new else d, p(held[3], m_new), p(held[4], m_new), m_new)
    outs = (_capi.ptr(out), stride, _capi.ptr(gid), _capi.ptr(inv), _capi.ptr(src_out), _capi.ptr(uniq), _capi.ptr(offs), _capi.ptr(nb))
    if dst == "sq8":
        _capi.check(L.nlsh_csr_update_sq8(p(old[0], n_old), _capi.ptr(quant[0]), _capi.ptr(quant[1]), *index, _capi.ptr(rows), CODE[src], *new, *outs,
                                          _capi.ptr(flags[0:1]), _capi.ptr(flags[1:2]), _capi.ptr(ws), wb, _stream()))
    else:
        flags[1] = 0
        _capi.check(L.nlsh_csr_update_typed(p(old[0], n_old), CODE[dst], *index, _capi.ptr(rows), CODE[src], *new, *outs, _capi.ptr(flags[0:1]),
                                            _capi.ptr(ws), wb, _stream()))
    torch.cuda.synchronize()
    b = int(nb.item())
    bad, clamped = flags.cpu().tolist()
    return out, inv, gid, src_out, uniq[:b], offs[:b + 1], bad, clamped


def stored_by_rule(values, src, dst, d, quant):
    """What `dst` holds of the float32 `values` [n, d] (exact in `src`), by the storage's rule and without the library -> [n, pitch]."""
    out = torch.zeros((values.shape[0], pitch(dst, d)), dtype=TORCH[dst], device="cuda")
    if dst == "sq8" and src != "uint8":         # code = clamp(rint((x - lo) / step), 0, 255): IEEE float32 subtract and divide, ties to even
        lo, step = quant[0][:d].cpu().numpy(), quant[1][:d].cpu().numpy()
        values = np.clip(np.rint((values - lo) / step), 0, 255)
    out[:, :d] = dev(values.astype(np.float32)).to(TORCH[dst])
    return out


def float32_inv_norm(stored, dst, d, quant):
    """`nlsh_gather_rows` (identity order, the float32 default pitch) on the dequantised rows -> inv_norm."""
    n, s4 = stored.shape[0], (d + 3) // 4 * 4
    deq = stored[:, :d].float()
    if dst == "sq8":
        deq = deq * quant[1][:d] + quant[0][:d]             # two roundings, as the rule says
    deq = deq.contiguous()
    ref, inv = torch.empty((n, s4), dtype=torch.float32, device="cuda"), torch.empty((n,), dtype=torch.float32, device="cuda")
    ident = torch.arange(n, dtype=torch.int32, device="cuda")
    _capi.check(_capi.lib().nlsh_gather_rows(_capi.ptr(deq), d, d, _capi.ptr(ident), n, _capi.ptr(ref), s4, _capi.ptr(inv), None, 0, _stream()))
    return inv


@pytest.mark.parametrize("d", DIMS)
def test_an_update_is_the_gather_built_rebuild(d):
    rng = np.random.default_rng(100 + d)
    for src in SOURCES:
        for dst in DESTINATIONS:
            quant = quantiser(dst, d, rng)
            for n_old, m_new, layout in [(n, m, lay) for n in (0, 5) for m in (0, 37) for lay in ("aligned", "offset") if m or lay == "aligned"]:
                what = (src, dst, d, n_old, m_new, layout)
                O = rng.integers(0, 256, size=(n_old, d)).astype(np.float32)
                R = rng.integers(0, 256, size=(m_new, d)).astype(np.float32)
                keys_old, keys_new = rng.integers(-3, 4, size=n_old).astype(np.int32), rng.integers(-3, 4, size=m_new).astype(np.int32)
                ids_new = np.arange(1000, 1000 + m_new, dtype=np.int32)
                # the index that is updated: gather-built, its rows' ids their local numbers; sorted rows 1 and 3 are removed
                perm_old, uniq_old, offs_old = csr(keys_old)
                old = gather(laid_out(O, src, "aligned"), src, dst, d, perm_old, quant) if n_old else (None, None, None, -1, 0)
                assert old[3:] == (-1, 0), what
                keep = np.ones(n_old, bool)
                keep[np.array([1, 3][:n_old], dtype=np.int64)] = False
                got = update(old, uniq_old, offs_old, keep, laid_out(R, src, layout), src, dst, d, keys_new, ids_new, quant)
                assert got[6:] == (-1, 0), what
                # the rebuild: the kept rows in local order, then the new ones
                kept = np.sort(perm_old[keep])
                n_kept = len(kept)
                rows_all, keys_all = np.concatenate([O[kept], R]), np.concatenate([keys_old[kept], keys_new])
                ids_all = np.concatenate([kept.astype(np.int32), ids_new])
                perm_all, uniq_all, offs_all = csr(keys_all)
                if n_kept + m_new == 0:
                    assert got[4].numel() == 0 and got[5].cpu().tolist() == [0], what
                    continue
                want = gather(laid_out(rows_all, src, "aligned"), src, dst, d, perm_all, quant)
                assert want[3:] == (-1, 0), what
                _same(want[0], stored_by_rule(rows_all[perm_all], src, dst, d, quant), (what, "gathered rows against the storage's rule"))
                off = gather(laid_out(rows_all, src, "offset"), src, dst, d, perm_all, quant)        # the element-load path of the gather
                assert off[3:] == (-1, 0), what
                for i, name in enumerate(("rows", "inv_norm", "gid")):
                    _same(off[i], want[i], (what, "gather from the offset source", name))
                _same(got[0], want[0], (what, "rows"))
                _same(got[1], want[1], (what, "inv_norm"))
                _same(got[1], float32_inv_norm(got[0], dst, d, quant), (what, "inv_norm against the float32 gather"))
                assert torch.equal(got[2].cpu(), torch.from_numpy(ids_all[perm_all])), (what, "gid")
                pos_old = np.empty(n_old, np.int32)
                pos_old[perm_old] = np.arange(n_old, dtype=np.int32)
                src_want = np.where(perm_all < n_kept, pos_old[kept[np.minimum(perm_all, max(n_kept - 1, 0))]] if n_kept else 0, ~(perm_all - n_kept))
                assert torch.equal(got[3].cpu(), torch.from_numpy(src_want.astype(np.int32))), (what, "src")
                assert torch.equal(got[4].cpu(), torch.from_numpy(uniq_all)) and torch.equal(got[5].cpu(), torch.from_numpy(offs_all)), (what, "buckets")


# (source, destination) -> a value the destination refuses
REFUSED = {("float32", "float16"): 1e6, ("float32", "uint8"): 0.5, ("float16", "uint8"): 0.5, ("float32", "sq8"): np.nan, ("float16", "sq8"): np.nan}


@pytest.mark.parametrize("d", DIMS)
def test_first_bad_is_the_smallest_planted_row_and_saturated_rows_count_once(d):
    rng = np.random.default_rng(200 + d)
    n_old, m = 5, 37
    for src in SOURCES:
        for dst in DESTINATIONS:
            quant = quantiser(dst, d, rng)
            R = rng.integers(0, 256, size=(m, d)).astype(np.float32)
            want_bad, want_clamped = -1, 0
            if (src, dst) in REFUSED:
                R[23, d // 2] = R[11, d - 1] = REFUSED[src, dst]
                want_bad = 11
            if dst == "sq8" and src != "uint8":
                # rows 2 and 30 saturate, row 2 at both ends and (d > 4) in two chunks; so does the refused row 11, which is not counted
                R[2, 0], R[2, d - 1], R[30, d // 2] = 1e4, -1e4, 1e4
                if d > 1:
                    R[11, 0] = -1e4
                want_clamped = 2
            what = (src, dst, d)
            perm = rng.permutation(m).astype(np.int32)
            for layout in ("aligned", "offset"):
                got = gather(laid_out(R, src, layout), src, dst, d, perm, quant)
                assert got[3:] == (want_bad, want_clamped), (what, "gather", layout, got[3:])
            O = rng.integers(0, 256, size=(n_old, d)).astype(np.float32)
            keys_old, keys_new = rng.integers(-3, 4, size=n_old).astype(np.int32), rng.integers(-3, 4, size=m).astype(np.int32)
            perm_old, uniq_old, offs_old = csr(keys_old)
            old = gather(laid_out(O, src, "aligned"), src, dst, d, perm_old, quant)
            keep = np.ones(n_old, bool)
            keep[[1, 3]] = False
            for layout in ("aligned", "offset"):
                got = update(old, uniq_old, offs_old, keep, laid_out(R, src, layout), src, dst, d, keys_new, np.arange(1000, 1000 + m, dtype=np.int32), quant)
                assert got[6:] == (want_bad, want_clamped), (what, "update", layout, got[6:])
