"""Pure-numpy model of `nlsh_csr_update`'s placement (include/nlsh_hip.h): the merge rule evaluated literally (`merge`) and the rebuild
it must equal (`rebuild`: a stable sort of the kept rows' keys followed by the new rows' keys), which the CPU tests hold against each
other.  Keys are signed int32, ascending; rows are named by their ids."""
import numpy as np


def build(keys):
    """keys [n] in local order -> (perm, uniq, offs): the CSR of `nlsh_build_csr` (stable sort, signed order)."""
    keys = np.asarray(keys, dtype=np.int32)
    perm = np.argsort(keys, kind="stable").astype(np.int64)
    sk = keys[perm]
    heads = np.nonzero(np.r_[True, sk[1:] != sk[:-1]])[0] if len(sk) else np.zeros((0,), dtype=np.int64)
    return perm, sk[heads], np.r_[heads, len(sk)].astype(np.int64)


def rebuild(keys_old, ids_old, remove, keys_new, ids_new):
    """The oracle: the index built from the surviving old rows in local order followed by the new rows -> (ids, keys) at every sorted
    position, (uniq, offs)."""
    keys_old, ids_old = np.asarray(keys_old, dtype=np.int32), np.asarray(ids_old, dtype=np.int64)
    stay = ~np.isin(ids_old, np.asarray(remove, dtype=np.int64))
    keys = np.r_[keys_old[stay], np.asarray(keys_new, dtype=np.int32)].astype(np.int32)
    ids = np.r_[ids_old[stay], np.asarray(ids_new, dtype=np.int64)]
    perm, uniq, offs = build(keys)
    return ids[perm], keys[perm], uniq, offs


def merge(uniq_old, offs_old, gid_old, keep, keys_new, ids_new):
    """The merge rule on an index in sorted order (uniq_old [nb], offs_old [nb + 1], gid_old [N]; keep [N] bool in sorted order)
    -> (ids, keys, src) at every destination and the run-length encoding (uniq, offs) of the keys.  src: the old sorted position, or
    ~j for new row j."""
    uniq_old, offs_old = np.asarray(uniq_old, dtype=np.int32), np.asarray(offs_old, dtype=np.int64)
    gid_old, keep = np.asarray(gid_old, dtype=np.int64), np.asarray(keep, dtype=bool)
    keys_new, ids_new = np.asarray(keys_new, dtype=np.int32), np.asarray(ids_new, dtype=np.int64)
    N, M = len(gid_old), len(keys_new)
    kex = np.r_[0, np.cumsum(keep)].astype(np.int64)            # kex[N] = rows kept
    perm_n, uniq_n, offs_n = build(keys_new)
    n_out = int(kex[N]) + M
    ids, keys, src = (np.full((n_out,), -1, dtype=np.int64), np.zeros((n_out,), dtype=np.int32), np.zeros((n_out,), dtype=np.int64))
    written = np.zeros((n_out,), dtype=bool)
    for b in range(len(uniq_old)):                              # kept old rows: behind every new row with a smaller key
        shift = int(offs_n[np.searchsorted(uniq_n, uniq_old[b], side="left")])
        for i in range(int(offs_old[b]), int(offs_old[b + 1])):
            if keep[i]:
                dst = int(kex[i]) + shift
                assert not written[dst]
                ids[dst], keys[dst], src[dst], written[dst] = gid_old[i], uniq_old[b], i, True
    for c in range(len(uniq_n)):                                # new rows: behind every kept old row with a key up to theirs
        shift = int(kex[offs_old[np.searchsorted(uniq_old, uniq_n[c], side="right")]]) if N else 0
        for t in range(int(offs_n[c]), int(offs_n[c + 1])):
            dst = t + shift
            assert not written[dst]
            ids[dst], keys[dst], src[dst], written[dst] = ids_new[perm_n[t]], uniq_n[c], ~int(perm_n[t]), True
    assert written.all()
    heads = np.nonzero(np.r_[True, keys[1:] != keys[:-1]])[0] if n_out else np.zeros((0,), dtype=np.int64)
    return ids, keys, src, keys[heads], np.r_[heads, n_out].astype(np.int64)
