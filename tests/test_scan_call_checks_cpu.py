"""The one argument check of a scan call (`scan_call_check`, csrc/scan_topk.hip) through all seven C entry points that describe one:
`nlsh_scan_topk`, `_phase`, `_cells_phase`, `_cells_phase_typed`, `_cells_phase_filtered`, `nlsh_range_count` and `nlsh_range_fill`.
Every entry is driven from ONE valid argument set; every case makes exactly one thing wrong and asserts the return code and that the
message names the argument (or its value).  No call reaches a device: the pointers are made-up aligned addresses that a refused call
never reads, and the valid set itself ends at the last host check (a workspace of 0 bytes: NLSH_E_WORKSPACE).

The expected codes are literals recorded from the library of the commit BEFORE the entry points shared one check (loaded beside this one
with NLSH_HIP_LIB): the refactor may not change the code of any call with one fault.  Where entries disagreed then, they disagree here:
`d` beyond NLSH_MAX_DIM on a float16 / uint8 top-k call is NLSH_E_INVALID (its pitch, held first, is then shorter than d) and
NLSH_E_UNSUPPORTED everywhere else."""
import pytest

from nlsh_amd import _capi

OK, INVALID, UNSUPPORTED, WORKSPACE = _capi.OK, _capi.E_INVALID, _capi.E_UNSUPPORTED, _capi.E_WORKSPACE
F32, F16, U8 = _capi.STORE_F32, _capi.STORE_F16, _capi.STORE_U8
QUERY, BUCKET, TILED = _capi.SCAN_QUERY_MAJOR, _capi.SCAN_BUCKET_MAJOR, _capi.SCAN_BUCKET_TILED
FAKE = 0x10000          # a 256-byte aligned non-null address: refused calls never dereference it

_HEAD = ("corpus_sorted", "row_stride", "d", "gid", "uniq_keys", "offsets", "bucket_order", "n_buckets")
_CELLS = ("cell_of", "cell_offsets", "n_cells")
_QUERIES = ("inv_norm", "queries", "q_stride", "Q", "qkeys", "nkeys", "P")
_TOPK = _QUERIES + ("k", "metric", "algo", "seg_rows", "out_dist", "out_idx", "out_keys", "out_ncand", "status", "workspace", "workspace_bytes",
                    "max_tasks", "ev_scan_begin", "ev_scan_end", "stream")
_TYPED_HEAD = _HEAD[:1] + ("storage",) + _HEAD[1:]
_RANGE = _TYPED_HEAD + _CELLS + _QUERIES + ("metric", "algo", "row_filter", "radius")
_RANGE_TAIL = ("status", "workspace", "workspace_bytes", "max_tasks")
_EVENTS = ("ev_scan_begin", "ev_scan_end", "stream")
ENTRIES = {      # entry -> (symbol, its parameters in order)
    "scan_topk": ("nlsh_scan_topk", _HEAD + _TOPK),
    "phase": ("nlsh_scan_topk_phase", _HEAD + _TOPK + ("phases",)),
    "cells": ("nlsh_scan_topk_cells_phase", _HEAD + _CELLS + _TOPK + ("phases",)),
    "typed": ("nlsh_scan_topk_cells_phase_typed", _TYPED_HEAD + _CELLS + _TOPK + ("phases",)),
    "filtered": ("nlsh_scan_topk_cells_phase_filtered", _TYPED_HEAD + _CELLS + _TOPK + ("phases", "row_filter")),
    "range_count": ("nlsh_range_count", _RANGE + ("out_count", "out_ncand") + _RANGE_TAIL + _EVENTS),
    "range_fill": ("nlsh_range_fill", _RANGE + ("row_offsets", "total", "cursor", "out_keys", "out_dist", "out_idx") + _RANGE_TAIL +
                   ("sort_workspace", "sort_workspace_bytes") + _EVENTS),
}
TOPK = ("scan_topk", "phase", "cells", "typed", "filtered")
RANGE = ("range_count", "range_fill")
STORED = ("typed", "filtered") + RANGE          # the entries with a storage argument

# The valid set: d = 100 in rows of 112 elements (a pitch of whole 16-byte units in every storage), the tiled schedule, a filter wherever
# there is a parameter for one.  What an entry has no parameter for is what the header says the entry implies.
VALID = dict(corpus_sorted=FAKE, storage=F32, row_stride=112, d=100, gid=FAKE, uniq_keys=FAKE, offsets=FAKE, bucket_order=None, n_buckets=3,
             cell_of=None, cell_offsets=None, n_cells=0, inv_norm=None, queries=FAKE, q_stride=100, Q=4, qkeys=FAKE, nkeys=FAKE, P=2, k=10,
             metric=_capi.METRIC_L2_EPS, algo=TILED, seg_rows=0, out_dist=FAKE, out_idx=FAKE, out_keys=None, out_ncand=FAKE, status=FAKE,
             workspace=FAKE, workspace_bytes=0, max_tasks=16, ev_scan_begin=None, ev_scan_end=None, stream=None, phases=_capi.PHASE_ALL,
             row_filter=FAKE, radius=FAKE, out_count=FAKE, row_offsets=FAKE, total=5, cursor=FAKE, sort_workspace=FAKE, sort_workspace_bytes=0)
IMPLIED = dict(storage=F32, row_filter=None)    # overrides an entry without the parameter still takes: they say what it already is

_NO_FILTER = dict(row_filter=None)              # the two other schedules are valid only without a filter
_SHARED_POINTERS = ("queries", "qkeys", "nkeys", "status", "workspace", "corpus_sorted", "gid", "uniq_keys", "offsets")

# (fault, what is made wrong, a fragment of the message, the entries it applies to -- None: every entry with these parameters)
FAULTS = [
    ("Q negative", dict(Q=-1), "Q=-1", None),
    ("Q = 2^31", dict(Q=1 << 31), "Q=2147483648", None),
    ("d = 0", dict(d=0), "d=0", None),
    ("d > MAX_DIM", dict(d=_capi.MAX_DIM + 1, row_stride=1040, q_stride=_capi.MAX_DIM + 1), "d=1025", None),
    ("d > MAX_DIM, float16", dict(d=_capi.MAX_DIM + 1, storage=F16), "d=1025", STORED),       # the pitch and q_stride stay: both are < d now
    ("P = 0", dict(P=0), "P=0", None),
    ("P > MAX_PROBES", dict(P=_capi.MAX_PROBES + 1), "P=65", None),
    ("k = 0", dict(k=0), "k=0", TOPK),
    ("k = 65, query-major", dict(k=65, algo=QUERY, **_NO_FILTER), "k=65", TOPK),
    ("k = 65, bucket-major", dict(k=65, algo=BUCKET, **_NO_FILTER), "k=65", TOPK),
    ("k = 257, tiled", dict(k=257), "k=257", TOPK),
    ("metric", dict(metric=9), "metric=9", None),
    ("algo", dict(algo=9), "algo=9", None),
    ("n_buckets negative", dict(n_buckets=-1), "n_buckets", None),
    ("max_tasks negative", dict(max_tasks=-1), "max_tasks", None),
    ("n_cells > n_buckets", dict(n_cells=4, cell_of=FAKE, cell_offsets=FAKE), "n_cells=4", None),
    ("cells without cell_of", dict(n_cells=2, cell_offsets=FAKE), "cell_of", None),
    ("cells without cell_offsets", dict(n_cells=2, cell_of=FAKE), "cell_offsets", None),
] + [("null " + name, {name: None}, "null", None) for name in _SHARED_POINTERS] + [
    ("null " + name, {name: None}, "null", TOPK) for name in ("out_dist", "out_idx", "out_ncand")
] + [
    ("cosine without inv_norm", dict(metric=_capi.METRIC_COSINE), "inv_norm", None),
    ("row_stride < d", dict(row_stride=96), "row_stride=96", None),
    ("pitch, float32", dict(row_stride=102), "multiple of 4", None),
    ("pitch, float16", dict(storage=F16, row_stride=100), "multiple of 8", STORED),
    ("pitch, uint8", dict(storage=U8, row_stride=104), "multiple of 16", STORED),
    ("corpus misaligned", dict(corpus_sorted=FAKE + 4), "16-byte aligned", None),
    ("corpus misaligned, float16", dict(corpus_sorted=FAKE + 8, storage=F16), "16-byte aligned", STORED),
    ("workspace misaligned", dict(workspace=FAKE + 4), "16-byte aligned", None),
    ("out_keys misaligned", dict(out_keys=FAKE + 4), "out_keys", None),
    ("row_filter misaligned", dict(row_filter=FAKE + 2), "row_filter", None),
    ("q_stride < d", dict(q_stride=99), "q_stride", None),
    ("phases = 0", dict(phases=0), "phases=0", None),
    ("phases: the internal bit", dict(phases=8), "phases=8", None),
    ("storage", dict(storage=7), "storage=7", None),
    ("float16, query-major", dict(storage=F16, algo=QUERY, **_NO_FILTER), "NLSH_SCAN_BUCKET_TILED", ("typed", "filtered")),
    ("uint8, bucket-major", dict(storage=U8, algo=BUCKET, **_NO_FILTER), "NLSH_SCAN_BUCKET_TILED", ("typed", "filtered")),
    ("filter, query-major", dict(algo=QUERY), "row_filter", ("filtered",)),
    ("filter, bucket-major", dict(algo=BUCKET), "row_filter", ("filtered",)),
    ("range, query-major", dict(algo=QUERY, **_NO_FILTER), "NLSH_SCAN_BUCKET_TILED", RANGE),
    ("range, bucket-major", dict(algo=BUCKET, **_NO_FILTER), "NLSH_SCAN_BUCKET_TILED", RANGE),
]

# fault -> the code every entry returns, or {entry: code} where they differ
CODES = {
    "Q negative": INVALID, "Q = 2^31": INVALID, "d = 0": UNSUPPORTED, "d > MAX_DIM": UNSUPPORTED,
    "d > MAX_DIM, float16": {"typed": INVALID, "filtered": INVALID, "range_count": UNSUPPORTED, "range_fill": UNSUPPORTED},
    "P = 0": UNSUPPORTED, "P > MAX_PROBES": UNSUPPORTED, "k = 0": UNSUPPORTED, "k = 65, query-major": UNSUPPORTED,
    "k = 65, bucket-major": UNSUPPORTED, "k = 257, tiled": UNSUPPORTED, "metric": INVALID, "algo": INVALID, "n_buckets negative": INVALID,
    "max_tasks negative": INVALID, "n_cells > n_buckets": INVALID, "cells without cell_of": INVALID, "cells without cell_offsets": INVALID,
    "cosine without inv_norm": INVALID, "row_stride < d": INVALID, "pitch, float32": INVALID, "pitch, float16": INVALID, "pitch, uint8": INVALID,
    "corpus misaligned": INVALID, "corpus misaligned, float16": INVALID, "workspace misaligned": INVALID, "out_keys misaligned": INVALID,
    "row_filter misaligned": INVALID, "q_stride < d": INVALID, "phases = 0": INVALID, "phases: the internal bit": INVALID, "storage": INVALID,
    "float16, query-major": UNSUPPORTED, "uint8, bucket-major": UNSUPPORTED, "filter, query-major": UNSUPPORTED,
    "filter, bucket-major": UNSUPPORTED, "range, query-major": UNSUPPORTED, "range, bucket-major": UNSUPPORTED,
}
CODES.update({"null " + name: INVALID for name in _SHARED_POINTERS + ("out_dist", "out_idx", "out_ncand")})


def applies(entry, overrides, only):
    params = ENTRIES[entry][1]
    if only is not None and entry not in only:
        return False
    return all(name in params or (name in IMPLIED and IMPLIED[name] == value) for name, value in overrides.items())


def call(entry, **overrides):
    symbol, params = ENTRIES[entry]
    values = {**VALID, **overrides}
    rc = getattr(_capi.lib(), symbol)(*[values[name] for name in params])
    return rc, _capi.lib().nlsh_last_error().decode()


CASES = [(entry, fault) for fault, overrides, _, only in FAULTS for entry in ENTRIES if applies(entry, overrides, only)]


def test_the_table_covers_every_entry_and_every_fault():
    assert {f[0] for f in FAULTS} == set(CODES) and len(FAULTS) == len(CODES)
    for entry, (symbol, params) in ENTRIES.items():
        assert len(getattr(_capi.lib(), symbol).argtypes) == len(params), entry           # the parameter lists above are the binding's
        assert sum(e == entry for e, _ in CASES) >= 30, entry
    assert all(any(f == fault for _, f in CASES) for fault in CODES)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_the_valid_set_passes_every_argument_check(entry):
    rc, msg = call(entry)
    assert rc == WORKSPACE and "workspace" in msg, (rc, msg)        # 0 bytes: the last host check, behind every check of the arguments
    if entry not in RANGE:                                            # ... on the other schedules too (top-k calls; without the filter)
        for algo in (QUERY, BUCKET):
            rc, msg = call(entry, algo=algo, row_filter=None)
            assert rc == WORKSPACE and "workspace" in msg, (algo, rc, msg)


@pytest.mark.parametrize("entry, fault", CASES)
def test_one_fault_one_code_and_the_argument_named(entry, fault):
    overrides, fragment = next((o, frag) for f, o, frag, _ in FAULTS if f == fault)
    want = CODES[fault][entry] if isinstance(CODES[fault], dict) else CODES[fault]
    rc, msg = call(entry, **overrides)
    assert rc == want, (rc, msg)
    if fault == "d > MAX_DIM, float16" and want == INVALID:
        fragment = "row_stride=112"        # the pitch is what this entry names: it is shorter than d
    assert fragment in msg, msg
    prefix = {"scan_topk": "scan_topk:", "phase": "scan_topk_phase:", "cells": "scan_topk_cells_phase:", "typed": "scan_topk_typed:",
              "filtered": "scan_topk_filtered:" if overrides.get("row_filter", FAKE) else "scan_topk_typed:",
              "range_count": "range_count:", "range_fill": "range_fill:"}[entry]
    assert msg.startswith(prefix), msg                                 # the entry that was called says so


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_an_empty_batch_is_valid_without_its_pointers(entry):
    """Q = 0: NLSH_OK with every device pointer null.  (The radius calls look at `radius`, `out_count` and `row_offsets` before they look
    at Q, as they always did: those three stay.)"""
    nulls = {name: None for name, value in VALID.items() if value == FAKE and name not in ("radius", "out_count", "row_offsets")}
    rc, msg = call(entry, Q=0, **nulls)
    assert rc == OK, (rc, msg)
    rc, msg = call(entry, Q=0, total=0, **nulls)
    assert rc == OK, (rc, msg)
