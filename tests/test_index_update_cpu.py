"""Index update (`nlsh_csr_update`, `Indexer.update`), the parts that need no device: the merge rule against the stable-sort rebuild
(tests/csr_update_ref.py), the symbols against the header, the workspace size as a function of its arguments and the host-side
argument checks (nothing is launched and no pointer is read before they pass)."""
import ctypes
import os
import re

import numpy as np
import pytest

import csr_update_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def L():
    from nlsh_amd import _capi
    return _capi.lib()


# ---------------------------------------------------------------------------------------------- the merge rule
def _case(rng, N, M, key_pool, remove_mode):
    keys_old = rng.choice(key_pool, size=N).astype(np.int32)
    ids_old = rng.permutation(4 * N + 8)[:N].astype(np.int64)
    keys_new = rng.choice(key_pool, size=M).astype(np.int32)
    ids_new = (4 * N + 8 + rng.permutation(4 * M + 8)[:M]).astype(np.int64)
    if remove_mode == "none":
        remove = np.zeros((0,), dtype=np.int64)
    elif remove_mode == "all":
        remove = ids_old.copy()
    else:   # some known ids (with repeats), some unknown ones
        known = rng.choice(ids_old, size=rng.integers(0, N + 1)) if N else np.zeros((0,), dtype=np.int64)
        remove = np.r_[known, rng.integers(10 ** 6, 10 ** 6 + 50, size=rng.integers(0, 4))].astype(np.int64)
    return keys_old, ids_old, remove, keys_new, ids_new


def _check(keys_old, ids_old, remove, keys_new, ids_new):
    perm, uniq, offs = ref.build(keys_old)
    gid = ids_old[perm]
    keep = ~np.isin(gid, remove)
    ids, keys, src, uniq_out, offs_out = ref.merge(uniq, offs, gid, keep, keys_new, ids_new)
    want_ids, want_keys, want_uniq, want_offs = ref.rebuild(keys_old, ids_old, remove, keys_new, ids_new)
    assert np.array_equal(ids, want_ids) and np.array_equal(keys, want_keys)
    assert np.array_equal(uniq_out, want_uniq) and np.array_equal(offs_out, want_offs)
    # src names where every row came from: an old sorted position, or ~j for new row j
    old = src >= 0
    assert np.array_equal(gid[src[old]], ids[old]) and np.array_equal(np.asarray(ids_new)[~src[~old]], ids[~old])
    assert np.all(np.diff(src[old]) > 0)            # kept old rows keep their order


def test_merge_rule_equals_the_stable_sort_rebuild_on_random_cases():
    rng = np.random.default_rng(20240611)
    pools = (np.arange(-3, 4), np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX]), np.arange(-50, 50), np.array([7]))
    for it in range(1500):
        N, M = int(rng.integers(0, 41)), int(rng.integers(0, 21))
        _check(*_case(rng, N, M, pools[it % len(pools)], ("none", "some", "some", "all")[it % 4 if it % 7 else 3]))


@pytest.mark.parametrize("N,M", [(0, 0), (0, 5), (5, 0), (1, 1), (40, 20)])
@pytest.mark.parametrize("remove_mode", ["none", "some", "all"])
def test_merge_rule_on_empty_sides_and_extreme_keys(N, M, remove_mode):
    rng = np.random.default_rng(N * 100 + M)
    _check(*_case(rng, N, M, np.array([I32_MIN, I32_MAX, 0]), remove_mode))


def test_merge_rule_layouts():
    ids = lambda n, base=0: np.arange(base, base + n, dtype=np.int64)   # noqa: E731
    old = np.repeat(np.array([10, 20, 30], dtype=np.int32), 4)
    for new in ([1, 2, 3], [40, 41], [5, 15, 25, 35], [10, 20, 30, 20], [25] * 6, [I32_MIN, I32_MAX]):
        _check(old, ids(12), [], np.array(new, dtype=np.int32), ids(len(new), 100))
        _check(old, ids(12), [0, 11, 4, 5, 6, 7, 999, 4], np.array(new, dtype=np.int32), ids(len(new), 100))


# ---------------------------------------------------------------------------------------------- the C ABI, host side
def test_header_symbols_and_library_agree_and_the_abi_is_still_4(L):
    from nlsh_amd import _capi
    header = open(os.path.join(ROOT, "include", "nlsh_hip.h")).read()
    for sym in ("nlsh_csr_update_workspace", "nlsh_csr_update"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in _capi.SYMBOLS
        assert getattr(L, sym).argtypes
    assert len(L.nlsh_csr_update.argtypes) == len(re.search(r"int nlsh_csr_update\((.*?)\);", header, re.S).group(1).split(","))
    assert int(re.search(r"#define NLSH_ABI_VERSION (\d+)", header).group(1)) == 4 and L.nlsh_abi_version() == 4


def test_workspace_is_zero_for_invalid_arguments(L):
    ws = L.nlsh_csr_update_workspace
    assert ws(0, 0, 0) > 0 and ws(1000, 10, 0) > 0 and ws(0, 0, 1000) > 0
    assert ws((1 << 31) - 1, 5, (1 << 31) - 1) > 0
    for n_old, nb, m in ((-1, 0, 0), (10, -1, 0), (10, 5, -1), (1 << 31, 5, 0), (10, 5, 1 << 31), (10, 11, 5)):
        assert ws(n_old, nb, m) == 0, (n_old, nb, m)
        assert "csr_update_workspace" in L.nlsh_last_error().decode()


def test_workspace_is_monotone_in_each_argument(L):
    ws = L.nlsh_csr_update_workspace
    counts = (0, 1, 63, 64, 65, 1000, 4097, 10 ** 6, 10 ** 8, (1 << 31) - 1)
    sizes = [ws(n, 0 if n == 0 else 1, 1000) for n in counts]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0], sizes
    sizes = [ws(10 ** 6, 1000, m) for m in counts]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0], sizes
    sizes = [ws(10 ** 6, nb, 1000) for nb in (0, 1, 64, 65, 1000, 65536, 10 ** 6)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0], sizes
    # O(M + n_buckets + 4 bytes x a few per row): nothing like a second corpus
    assert ws(10 ** 6, 65536, 1000) < 10 ** 6 * 24 + (4 << 20)


def _update(L, d=128, n_old=1000, nb_old=10, n_kept=None, keep=True, m_new=100, row_stride=None, new_stride=None, stride_out=None,
            ws_bytes=None, null=(), misalign=()):
    """nlsh_csr_update with pointers into a small host buffer: every call here must be refused before any of them is used."""
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255
    need = L.nlsh_csr_update_workspace(n_old, nb_old, m_new) or (1 << 20)
    p = lambda name: None if name in null else a + 4 if name in misalign else a   # noqa: E731
    return L.nlsh_csr_update(
        p("corpus_sorted"), d if row_stride is None else row_stride, d, p("gid"), p("inv_norm"), p("uniq_keys"), p("offsets"), n_old, nb_old,
        p("keep") if keep else None, (n_old if not keep or n_old < 1 else n_old - 1) if n_kept is None else n_kept,
        p("rows_new"), d if new_stride is None else new_stride, p("keys_new"), p("ids_new"), m_new,
        p("sorted_out"), d if stride_out is None else stride_out, p("gid_out"), p("inv_norm_out"), p("src_out"), p("uniq_out"),
        p("offsets_out"), p("n_buckets_out"), p("workspace"), need if ws_bytes is None else ws_bytes, None)


def test_every_host_side_refusal_is_e_invalid_and_names_the_argument(L):
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731

    def refused(name, **kw):
        assert _update(L, **kw) == _capi.E_INVALID, (name, kw)
        assert name in err(), (name, err())

    for d in (0, -3, 1025):
        refused(f"d={d}", d=d, row_stride=2048, new_stride=2048, stride_out=2048)
    assert "NLSH_MAX_DIM" in err()
    refused("row_stride=124", row_stride=124)             # < d
    refused("row_stride=130", row_stride=130)             # not a multiple of 4
    refused("new_stride=127", new_stride=127)
    refused("stride_out=127", stride_out=127)
    refused("stride_out=130", stride_out=130)
    refused("n_old=-1", n_old=-1)
    refused("n_old=%d" % (1 << 31), n_old=1 << 31)
    refused("m_new=-1", m_new=-1)
    refused("m_new=%d" % (1 << 31), m_new=1 << 31)
    refused("n_buckets_old=-1", nb_old=-1)
    refused("n_buckets_old=1001", nb_old=1001)
    refused("n_buckets_old=0", nb_old=0)                  # rows without a bucket
    refused("n_kept=-1", n_kept=-1)
    refused("n_kept=1001", n_kept=1001)
    refused("n_kept=999", keep=False, n_kept=999)         # no keep array = every row kept
    refused("2^31 - 1", n_old=(1 << 31) - 1, nb_old=1, keep=False, m_new=1)     # the int32 row bound
    for name in ("corpus_sorted", "gid", "uniq_keys", "offsets", "rows_new", "keys_new", "ids_new", "sorted_out", "gid_out", "src_out",
                 "uniq_out", "offsets_out", "n_buckets_out", "workspace"):
        refused(name, null=(name,))
    refused("inv_norm", null=("inv_norm",))               # inv_norm_out wanted, the kept rows' inv_norm missing
    for name in ("corpus_sorted", "sorted_out", "workspace"):
        refused(name, misalign=(name,))
        assert "16-byte aligned" in err()
    need = L.nlsh_csr_update_workspace(1000, 10, 100)
    for have in (0, 16, need - 1):
        refused("workspace_bytes", ws_bytes=have)
        assert str(need) in err() and str(have) in err() and "nlsh_csr_update_workspace" in err()


def test_nullable_arguments_are_only_needed_where_they_are_read(L):
    """No new rows: no new arrays (nor `inv_norm` without `inv_norm_out`); no old rows: no old arrays.  Each call passes every pointer
    check and is stopped by the LAST host check, the workspace size, so nothing reaches a device."""
    from nlsh_amd import _capi
    err = lambda: L.nlsh_last_error().decode()   # noqa: E731
    rc = _update(L, m_new=0, null=("rows_new", "keys_new", "ids_new", "inv_norm", "inv_norm_out"), ws_bytes=0)
    assert rc == _capi.E_INVALID and "workspace_bytes" in err()
    rc = _update(L, n_old=0, nb_old=0, keep=False, null=("corpus_sorted", "gid", "inv_norm", "uniq_keys", "offsets", "keep"), ws_bytes=0)
    assert rc == _capi.E_INVALID and "workspace_bytes" in err()


def test_facade_refuses_before_touching_a_device():
    """`update`'s argument checks on an Indexer that never saw a device (built by hand: the constructor needs one)."""
    import torch
    from nlsh_amd import _capi
    from nlsh_amd.indexer import Indexer
    ix = Indexer.__new__(Indexer)
    ix.metric = "custom"
    with pytest.raises(NotImplementedError, match="generic-metric"):
        ix.update(add=torch.zeros(2, 4))
    with pytest.raises(NotImplementedError):
        ix.remove([1])
    ix.metric, ix.dim, ix.row_ids = "l2", 4, None
    with pytest.raises(_capi.NlshHipError) as e:
        ix._new_rows(torch.zeros(2, 4), None, None, torch.device("cuda", 0))
    assert e.value.code == _capi.E_INVALID and "no CPU path" in str(e.value)
    with pytest.raises(ValueError, match="without rows"):
        ix._new_rows(None, [1, 2], None, torch.device("cuda", 0))
