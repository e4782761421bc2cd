"""The one argument check of a row call (`row_call_check`, csrc/build_csr.hip) through the six C entry points that describe one --
`nlsh_gather_rows`, `_typed`, `_sq8` and `nlsh_csr_update`, `_typed`, `_sq8` -- and `nlsh_sq8_train`'s own beside them.  Every entry is
driven from ONE valid argument set of its family (d = 100 in rows of 112 elements, a pitch of whole 16-byte units in every storage);
every case makes exactly one thing wrong and asserts the return code and that the message names the argument (or its value).  No call
reaches a device: the pointers are made-up aligned addresses that a refused call never reads.  The valid sets themselves are not
called: they would be enqueued.

The expected codes are literals recorded from the library of the commit BEFORE the entry points shared one check (built beside this
one and loaded with NLSH_HIP_LIB): the refactor may not change the code of any call with one fault.  Where entries disagreed then, they
disagree here:
  * a short workspace is NLSH_E_INVALID for the three updates and NLSH_E_WORKSPACE for `nlsh_sq8_train`;
  * `nlsh_gather_rows` does not hold `corpus` to its element size and the updates do not hold `rows_new` to theirs (such a call is
    enqueued, so it is not made here); the typed and sq8 gathers and the training call refuse a misaligned element pointer;
  * `nlsh_csr_update_sq8` holds its two pitches against each other before anything else, under its own name: `stride_out` alone below
    d is "row_stride != stride_out" there and "stride_out=96" in the two other updates;
  * the updates hold `lo` / `step` whatever the row counts, `nlsh_gather_rows_sq8` only when there are rows; a converting gather wants
    `first_bad` even for no rows, a converting update only with new rows."""
import pytest

from nlsh_amd import _capi

OK, INVALID, WORKSPACE = _capi.OK, _capi.E_INVALID, _capi.E_WORKSPACE
F32, F16, U8 = _capi.STORE_F32, _capi.STORE_F16, _capi.STORE_U8
FAKE = 0x10000          # a 256-byte aligned non-null address: refused calls never dereference it
NEED = "need"           # workspace_bytes: what the entry's workspace query returns for the call's counts

_G_HEAD = ("corpus", "src_stride", "d", "perm", "n", "sorted")
_G_TYPED_HEAD = ("corpus", "src_storage", "src_stride", "d", "perm", "n", "sorted")
_G_OUT = ("inv_norm", "gid", "id_base")
_U_OLD = ("row_stride", "d", "gid", "inv_norm", "uniq_keys", "offsets", "n_old", "n_buckets_old", "keep", "n_kept")
_U_NEW = ("new_stride", "keys_new", "ids_new", "m_new")
_U_OUT = ("sorted_out", "stride_out", "gid_out", "inv_norm_out", "src_out", "uniq_out", "offsets_out", "n_buckets_out")
_U_WS = ("workspace", "workspace_bytes", "stream")
ENTRIES = {      # entry -> (symbol, its parameters in order, the prefix of its messages)
    "gather": ("nlsh_gather_rows", _G_HEAD + ("dst_stride",) + _G_OUT + ("stream",), "gather_rows:"),
    "gather_typed": ("nlsh_gather_rows_typed", _G_TYPED_HEAD + ("dst_storage", "dst_stride") + _G_OUT + ("first_bad", "stream"), "gather_rows_typed:"),
    "gather_sq8": ("nlsh_gather_rows_sq8", _G_TYPED_HEAD + ("dst_stride", "lo", "step") + _G_OUT + ("first_bad", "clamped_rows", "stream"),
                   "gather_rows_sq8:"),
    "update": ("nlsh_csr_update", ("corpus_sorted",) + _U_OLD + ("rows_new",) + _U_NEW + _U_OUT + _U_WS, "csr_update:"),
    "update_typed": ("nlsh_csr_update_typed", ("corpus_sorted", "storage") + _U_OLD + ("rows_new", "new_storage") + _U_NEW + _U_OUT + ("first_bad",) + _U_WS,
                     "csr_update:"),
    "update_sq8": ("nlsh_csr_update_sq8", ("corpus_sorted", "lo", "step") + _U_OLD + ("rows_new", "new_storage") + _U_NEW + _U_OUT +
                   ("first_bad", "clamped_rows") + _U_WS, "csr_update:"),
    "train": ("nlsh_sq8_train", ("rows", "storage", "row_stride", "d", "n", "lo", "step", "quant_stride", "first_bad", "workspace", "workspace_bytes", "stream"),
              "sq8_train:"),
}
GATHERS, UPDATES = ("gather", "gather_typed", "gather_sq8"), ("update", "update_typed", "update_sq8")

# The valid sets.  A gather converts float32 rows (to float16 where it has a destination storage); an update removes 10 of 1000 rows and
# adds 100 float32 ones (to a float16 index where it has a storage).
VALID = {
    **{e: dict(corpus=FAKE, src_storage=F32, src_stride=100, d=100, perm=FAKE, n=10, sorted=FAKE, dst_storage=F16, dst_stride=112, lo=FAKE, step=FAKE,
               inv_norm=FAKE, gid=FAKE, id_base=0, first_bad=FAKE, clamped_rows=FAKE, stream=None) for e in GATHERS},
    **{e: dict(corpus_sorted=FAKE, storage=F16, lo=FAKE, step=FAKE, row_stride=112, d=100, gid=FAKE, inv_norm=FAKE, uniq_keys=FAKE, offsets=FAKE, n_old=1000,
               n_buckets_old=10, keep=FAKE, n_kept=990, rows_new=FAKE, new_storage=F32, new_stride=100, keys_new=FAKE, ids_new=FAKE, m_new=100,
               sorted_out=FAKE, stride_out=112, gid_out=FAKE, inv_norm_out=FAKE, src_out=FAKE, uniq_out=FAKE, offsets_out=FAKE, n_buckets_out=FAKE,
               first_bad=FAKE, clamped_rows=FAKE, workspace=FAKE, workspace_bytes=NEED, stream=None) for e in UPDATES},
    "train": dict(rows=FAKE, storage=F32, row_stride=100, d=100, n=1000, lo=FAKE, step=FAKE, quant_stride=112, first_bad=FAKE, workspace=FAKE,
                  workspace_bytes=NEED, stream=None),
}

_U_POINTERS = ("corpus_sorted", "gid", "uniq_keys", "offsets", "rows_new", "keys_new", "ids_new", "sorted_out", "gid_out", "src_out", "uniq_out", "offsets_out",
               "n_buckets_out", "workspace")

# (fault, what is made wrong, a fragment of the message, the entries it applies to -- None: every entry with these parameters, the code)
FAULTS = [
    ("source storage", dict(src_storage=7), "src_storage=7", None, INVALID),
    ("destination storage", dict(dst_storage=7), "dst_storage=7", None, INVALID),
    ("destination storage: sq8 has entries of its own", dict(dst_storage=3), "dst_storage=3", None, INVALID),
    ("new rows' storage", dict(new_storage=7), "new_storage=7", None, INVALID),
    ("index storage", dict(storage=7), "storage=7", ("update_typed", "train"), INVALID),
    ("training on codes", dict(storage=U8), "storage=2", ("train",), INVALID),
    ("d = 0", dict(d=0), "d=0", None, INVALID),
    ("d > MAX_DIM", dict(d=_capi.MAX_DIM + 1), "d=1025", None, INVALID),
    ("n negative", dict(n=-1), "n=-1", None, INVALID),
    ("n_old negative", dict(n_old=-1), "n_old=-1", None, INVALID),
    ("n_old = 2^31", dict(n_old=1 << 31), "n_old=2147483648", None, INVALID),
    ("m_new negative", dict(m_new=-1), "m_new=-1", None, INVALID),
    ("n_kept negative", dict(n_kept=-1), "n_kept=-1", None, INVALID),
    ("n_kept > n_old", dict(n_kept=1001), "n_kept=1001", None, INVALID),
    ("null keep, n_kept != n_old", dict(keep=None), "keep is null", None, INVALID),
    ("n_buckets_old negative", dict(n_buckets_old=-1), "n_buckets_old=-1", None, INVALID),
    ("rows without a bucket", dict(n_buckets_old=0), "n_buckets_old=0", None, INVALID),
    ("dst_stride < d", dict(dst_stride=96), "dst_stride=96", None, INVALID),
    ("src_stride < d", dict(src_stride=99), "src_stride", None, INVALID),
    ("row_stride < d", dict(row_stride=96), "row_stride=96", ("update", "update_typed"), INVALID),
    ("stride_out < d", dict(stride_out=96), "stride_out=96", ("update", "update_typed"), INVALID),
    ("stride_out < d, sq8", dict(stride_out=96), "row_stride=112 != stride_out=96", ("update_sq8",), INVALID),
    ("both pitches < d, sq8", dict(row_stride=96, stride_out=96), "row_stride=96", ("update_sq8",), INVALID),
    ("new_stride < d", dict(new_stride=99), "new_stride=99", None, INVALID),
    ("training: row_stride < d", dict(row_stride=99), "row_stride=99", ("train",), INVALID),
    ("quant_stride < d", dict(quant_stride=96), "quant_stride=96", None, INVALID),
    ("pitch, float32 rows", dict(dst_stride=102), "multiple of 4", ("gather",), INVALID),
    ("pitch, to float32", dict(dst_storage=F32, src_storage=F16, dst_stride=102), "multiple of 4", None, INVALID),
    ("pitch, to float16", dict(dst_stride=100), "multiple of 8", ("gather_typed",), INVALID),
    ("pitch, to uint8", dict(dst_storage=U8, dst_stride=104), "multiple of 16", None, INVALID),
    ("pitch, to sq8", dict(dst_stride=104), "multiple of 16", ("gather_sq8",), INVALID),
    ("old pitch, float32 index", dict(row_stride=102), "multiple of 4", ("update",), INVALID),
    ("new pitch, float32 index", dict(stride_out=102), "multiple of 4", ("update",), INVALID),
    ("old pitch, float16 index", dict(row_stride=100), "multiple of 8", ("update_typed",), INVALID),
    ("new pitch, float16 index", dict(stride_out=100), "multiple of 8", ("update_typed",), INVALID),
    ("old pitch, uint8 index", dict(storage=U8, row_stride=104), "multiple of 16", ("update_typed",), INVALID),
    ("new pitch, uint8 index", dict(storage=U8, stride_out=104), "multiple of 16", ("update_typed",), INVALID),
    ("old pitch, float32 typed index", dict(storage=F32, new_storage=F16, row_stride=102), "multiple of 4", ("update_typed",), INVALID),
    ("pitches, sq8 index", dict(row_stride=104, stride_out=104), "multiple of 16", ("update_sq8",), INVALID),
    ("unequal sq8 pitches", dict(stride_out=128), "ONE pitch", ("update_sq8",), INVALID),
] + [("null " + name, {name: None}, "null", GATHERS, INVALID) for name in ("corpus", "perm", "sorted")] + [
    ("null " + name, {name: None}, name, UPDATES, INVALID) for name in _U_POINTERS
] + [("null " + name + ", training", {name: None}, "null", ("train",), INVALID) for name in ("rows", "lo", "step", "first_bad", "workspace")] + [
    ("null " + name, {name: None}, "lo / step is null", ("gather_sq8", "update_sq8"), INVALID) for name in ("lo", "step")
] + [
    ("null inv_norm of the kept rows", dict(inv_norm=None), "inv_norm", UPDATES, INVALID),
    ("null first_bad on a converting call", dict(first_bad=None), "first_bad", ("gather_typed", "gather_sq8", "update_typed", "update_sq8"), INVALID),
    ("sorted misaligned", dict(sorted=FAKE + 4), "16-byte aligned", None, INVALID),
    ("corpus_sorted misaligned", dict(corpus_sorted=FAKE + 4), "16-byte aligned", None, INVALID),
    ("sorted_out misaligned", dict(sorted_out=FAKE + 4), "16-byte aligned", None, INVALID),
    ("workspace misaligned", dict(workspace=FAKE + 4), "16-byte aligned", None, INVALID),
    ("lo misaligned", dict(lo=FAKE + 4), "lo and step must be 16-byte aligned", ("gather_sq8", "update_sq8"), INVALID),
    ("step misaligned", dict(step=FAKE + 4), "lo and step must be 16-byte aligned", ("gather_sq8", "update_sq8"), INVALID),
    ("float32 source off its element", dict(corpus=FAKE + 2), "element size", ("gather_typed", "gather_sq8"), INVALID),
    ("float16 source off its element", dict(corpus=FAKE + 1, src_storage=F16), "element size", ("gather_typed", "gather_sq8"), INVALID),
    ("training rows off their element", dict(rows=FAKE + 2), "element size", None, INVALID),
    ("short workspace", dict(workspace_bytes=-1), "workspace_bytes", UPDATES, INVALID),            # one byte less than NEED
    ("no workspace", dict(workspace_bytes=0), "workspace_bytes", UPDATES, INVALID),
    ("short workspace, training", dict(workspace_bytes=16), "workspace 16", ("train",), WORKSPACE),
]


def applies(entry, overrides, only):
    return (only is None or entry in only) and all(name in ENTRIES[entry][1] for name in overrides)


def call(entry, **overrides):
    symbol, params, _ = ENTRIES[entry]
    L = _capi.lib()
    values = {**VALID[entry], **overrides}
    if values.get("workspace_bytes") in (NEED, -1):
        need = (L.nlsh_sq8_train_workspace(values["n"], values["d"]) if entry == "train"
                else L.nlsh_csr_update_workspace(values["n_old"], values["n_buckets_old"], values["m_new"])) or (1 << 20)
        values["workspace_bytes"] = need if values["workspace_bytes"] == NEED else need - 1
    rc = getattr(L, symbol)(*[values[name] for name in params])
    return rc, L.nlsh_last_error().decode()


CASES = [(entry, fault) for fault, overrides, _, only, _ in FAULTS for entry in ENTRIES if applies(entry, overrides, only)]


def test_the_table_covers_every_entry_and_every_fault():
    assert len({f[0] for f in FAULTS}) == len(FAULTS)
    floor = {"gather": 10, "gather_typed": 18, "gather_sq8": 18, "update": 30, "update_typed": 35, "update_sq8": 35, "train": 14}
    for entry, (symbol, params, _) in ENTRIES.items():
        assert len(getattr(_capi.lib(), symbol).argtypes) == len(params), entry           # the parameter lists above are the binding's
        assert set(params) == set(VALID[entry]) & set(params) and sum(e == entry for e, _ in CASES) >= floor[entry], entry
    assert all(any(f == fault[0] for _, f in CASES) for fault in FAULTS)


@pytest.mark.parametrize("entry, fault", CASES)
def test_one_fault_one_code_and_the_argument_named(entry, fault):
    overrides, fragment, want = next((o, frag, code) for f, o, frag, _, code in FAULTS if f == fault)
    rc, msg = call(entry, **overrides)
    assert rc == want, (rc, msg)
    assert fragment in msg, msg
    prefix = "csr_update_sq8:" if "!=" in fragment or "ONE pitch" in fragment else ENTRIES[entry][2]
    assert msg.startswith(prefix), msg                                 # the entry that was called says so


@pytest.mark.parametrize("entry", GATHERS + ("train",))
def test_no_rows_need_no_row_pointers(entry):
    """n = 0: NLSH_OK without the pointers rows are read through -- nothing is launched for a gather.  (The flags such a call clears, and
    the training call, which writes the padding of lo / step, need a device: the gathers are made without flags here, codes to codes.)"""
    if entry == "train":
        rc, msg = call(entry, n=0, rows=None, workspace=None, lo=None)                 # ... but its outputs are held even then
        assert rc == INVALID and "null" in msg, (rc, msg)
        return
    nulls = dict(corpus=None, perm=None, sorted=None, lo=None, step=None, inv_norm=None, gid=None, first_bad=None, clamped_rows=None)
    same = dict(src_storage=U8, dst_storage=U8)
    rc, msg = call(entry, n=0, **{k: v for k, v in {**nulls, **same}.items() if k in ENTRIES[entry][1]})
    assert rc == OK, (rc, msg)


def test_a_converting_gather_of_no_rows_still_wants_first_bad_and_an_update_its_quantiser():
    for entry in ("gather_typed", "gather_sq8"):
        rc, msg = call(entry, n=0, first_bad=None)
        assert rc == INVALID and "first_bad" in msg, (entry, rc, msg)
    rc, msg = call("update_sq8", m_new=0, lo=None)
    assert rc == INVALID and "lo / step is null" in msg, (rc, msg)
    # an update without new rows converts nothing: no first_bad, and it is stopped by the last check, the workspace size
    for entry in ("update_typed", "update_sq8"):
        rc, msg = call(entry, m_new=0, first_bad=None, rows_new=None, keys_new=None, ids_new=None, workspace_bytes=0)
        assert rc == INVALID and "workspace_bytes" in msg, (entry, rc, msg)
