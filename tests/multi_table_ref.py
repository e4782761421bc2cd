"""The numpy reference of nlsh_merge_topk_unique and of a multi-table query -- numpy only, no GPU, no project kernel.

unique_merge_reference restates the call: per query, the first k keys of the G lists are concatenated, ~0 (padding) dropped, `np.unique`
on the uint64 keys (sorted, every key once), the first k kept, the tail padded with key ~0 / id -1 / dist +inf.  The candidate count is
the SUM over the lists, in nlsh_merge_topk's three forms.  tests/test_multi_table_cpu.py holds it against the definition it serves:
the unique merge of per-list top-k equals the top-k of the set union of the FULL lists."""
import numpy as np

import tie_ref as T

KEY_NONE = T.KEY_NONE
LOW32 = np.uint64(0xFFFFFFFF)


def split_keys(keys):
    """uint64 keys -> (dist float32, idx int32), ~0 -> (+inf, -1)."""
    keys = np.asarray(keys, dtype=np.uint64)
    none = keys == KEY_NONE
    dist = T.float_from_mono((keys >> np.uint64(32)).astype(np.uint32)).copy()
    idx = (keys & LOW32).astype(np.uint32).view(np.int32).copy()
    dist[none], idx[none] = np.inf, -1
    return dist, idx


def unique_merge_reference(keys_in, k):
    """keys_in uint64 [G, Q, row_stride >= k] -> (dist float32 [Q, k], idx int32 [Q, k], keys uint64 [Q, k])."""
    keys_in = np.asarray(keys_in, dtype=np.uint64)
    G, Q, _ = keys_in.shape
    out = np.full((Q, k), KEY_NONE, dtype=np.uint64)
    for q in range(Q):
        keys = keys_in[:, q, :k].reshape(-1)
        keys = np.unique(keys[keys != KEY_NONE])[:k]
        out[q, :len(keys)] = keys
    dist, idx = split_keys(out)
    return dist, idx, out


def union_topk(full_lists, k):
    """The DEFINITION: full_lists = the G complete candidate key sets of one query (uint64 arrays of any length, each distinct within
    itself) -> the k smallest keys of their set union, ~0 padded."""
    union = np.unique(np.concatenate([np.asarray(l, dtype=np.uint64) for l in full_lists] + [np.zeros(0, np.uint64)]))
    out = np.full(k, KEY_NONE, dtype=np.uint64)
    out[:min(k, len(union))] = union[:k]
    return out


def per_list_topk(full_lists, k, stride=None):
    """[G, stride] uint64: every list's own k smallest, ascending, ~0 padded (what one table's scan hands the merge)."""
    stride = k if stride is None else stride
    out = np.full((len(full_lists), stride), KEY_NONE, dtype=np.uint64)
    for g, l in enumerate(full_lists):
        s = np.sort(np.asarray(l, dtype=np.uint64))[:k]
        out[g, :len(s)] = s
    return out
