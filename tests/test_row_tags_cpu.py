"""Per-query tag filters without a device: the pass rule on hand-written words, every host-side refusal of the two new C
calls through the loaded library (no call reaches a device: made-up aligned addresses that a refused call never reads, as in
tests/test_scan_call_checks_cpu.py), the facade's refusals, and the generator of tests/row_tags_ref.py held against the world of
tests/test_gpu_row_filter.py, so that the GPU test cannot pass vacuously."""
import numpy as np
import pytest
import torch

import row_tags_ref as ref
from nlsh_amd import _capi
from test_scan_call_checks_cpu import _CELLS, _TOPK, _TYPED_HEAD, FAKE, VALID

OK, INVALID, UNSUPPORTED, WORKSPACE = _capi.OK, _capi.E_INVALID, _capi.E_UNSUPPORTED, _capi.E_WORKSPACE
U64 = np.uint64


# ---------------------------------------------------------------------------------------------- the rule
def test_the_pass_rule_on_hand_written_words():
    ones, b63, lo_half, hi_half = ref.ALL_ONES, U64(1 << 63), U64(0x00000000FFFFFFFF), U64(0xFFFFFFFF00000000)
    cases = [   # tag, mask, any, all, eq
        (0, 0, False, True, True), (0, ones, False, False, False), (ones, 0, False, True, False), (ones, ones, True, True, True),
        (b63, b63, True, True, True), (b63, U64(1), False, False, False), (U64(1), b63, False, False, False),
        (b63 | U64(1), b63, True, True, False), (b63, b63 | U64(1), True, False, False),
        (lo_half, hi_half, False, False, False), (lo_half, lo_half, True, True, True), (ones, hi_half, True, True, False),
        (U64(1 << 32), hi_half, True, False, False), (U64(1 << 31), lo_half, True, False, False), (U64(1 << 31), hi_half, False, False, False),
        (U64((1 << 31) | (1 << 32)), U64((1 << 31) | (1 << 32)), True, True, True), (U64(1 << 32), U64((1 << 31) | (1 << 32)), True, False, False),
        (0, b63, False, False, False), (ones, b63, True, True, False), (U64(0x7FFFFFFFFFFFFFFF), b63, False, False, False),
    ]
    for tag, mask, a, al, e in cases:
        got = tuple(bool(ref.passes(np.asarray([tag], dtype=U64), U64(mask), mode)[0]) for mode in ref.MODES)
        assert got == (a, al, e), (hex(int(tag)), hex(int(mask)), got)
    # arrays broadcast, and the signed container holds the same bits
    tags = np.asarray([0, 1, 1 << 63, 0xFFFFFFFFFFFFFFFF], dtype=U64)
    assert ref.passes(tags, ref.BIT63, "any").tolist() == [False, False, True, True]
    assert ref.as_i64(tags).tolist() == [0, 1, -(1 << 63), -1] and ref.as_i64(tags).view(U64).tolist() == tags.tolist()
    assert [_capi.TAG_ANY, _capi.TAG_ALL, _capi.TAG_EQ] == [0, 1, 2]
    from nlsh_amd.indexer import TAG_MATCH
    assert TAG_MATCH == {"any": 0, "all": 1, "eq": 2} and tuple(TAG_MATCH) == ref.MODES


# ---------------------------------------------------------------------------------------------- C ABI refusals
_TAIL = ("phases", "row_filter", "row_tags", "query_masks", "tag_match")
ENTRIES = {
    "tagged": ("nlsh_scan_topk_cells_phase_tagged", _TYPED_HEAD + _CELLS + _TOPK + _TAIL, "scan_topk_tagged:"),
    "sq8_tagged": ("nlsh_scan_topk_cells_phase_sq8_tagged", ("corpus_sorted", "lo", "step") + _TYPED_HEAD[2:] + _CELLS + _TOPK + _TAIL,
                   "scan_topk_sq8_tagged:"),
}
TAG_VALID = dict(VALID, lo=FAKE, step=FAKE, row_tags=FAKE, query_masks=FAKE, tag_match=_capi.TAG_ANY)
QUERY, BUCKET = _capi.SCAN_QUERY_MAJOR, _capi.SCAN_BUCKET_MAJOR


def _call(entry, **overrides):
    symbol, params, _ = ENTRIES[entry]
    values = {**TAG_VALID, **overrides}
    L = _capi.lib()
    assert len(getattr(L, symbol).argtypes) == len(params)
    rc = getattr(L, symbol)(*[values[name] for name in params])
    return rc, L.nlsh_last_error().decode()


FAULTS = [   # what is made wrong, the code, a fragment of the message
    (dict(algo=QUERY, row_filter=None), UNSUPPORTED, "row_tags"),
    (dict(algo=BUCKET, row_filter=None), UNSUPPORTED, "row_tags"),
    (dict(algo=QUERY, row_filter=None, row_tags=None), UNSUPPORTED, "query_masks"),
    (dict(row_tags=None), INVALID, "query_masks without row_tags"),
    (dict(query_masks=None), INVALID, "row_tags without query_masks"),
    (dict(row_tags=FAKE + 4), INVALID, "row_tags must be 8-byte aligned"),
    (dict(row_tags=FAKE + 1), INVALID, "row_tags must be 8-byte aligned"),
    (dict(query_masks=FAKE + 4), INVALID, "query_masks must be 8-byte aligned"),
    (dict(tag_match=3), INVALID, "tag_match=3"),
    (dict(tag_match=-1), INVALID, "tag_match=-1"),
    (dict(phases=8), INVALID, "phases=8"),                      # the internal plan-rest bit is not the C ABI's
    (dict(row_filter=FAKE + 2), INVALID, "row_filter"),         # the filtered call's refusals stay
    (dict(k=257), UNSUPPORTED, "k=257"),
]


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_host_side_refusal_of_the_tagged_calls(entry):
    prefix = ENTRIES[entry][2]
    if entry == "sq8_tagged":       # the uint8 pitch: rows of 112 elements
        assert TAG_VALID["row_stride"] % 16 == 0
    rc, msg = _call(entry)
    assert rc == WORKSPACE and "workspace" in msg, (rc, msg)          # the valid set ends at the last host check (0 bytes of workspace)
    for match in (_capi.TAG_ANY, _capi.TAG_ALL, _capi.TAG_EQ):
        rc, msg = _call(entry, tag_match=match, row_filter=None)
        assert rc == WORKSPACE, (match, rc, msg)
    for overrides, code, fragment in FAULTS:
        rc, msg = _call(entry, **overrides)
        assert rc == code and fragment in msg, (overrides, rc, msg)
        assert msg.startswith(prefix), msg
    # row_tags == NULL and query_masks == NULL: the base call, argument for argument -- tag_match is not looked at, the other schedules pass
    base = "scan_topk_sq8:" if entry == "sq8_tagged" else "scan_topk_filtered:"
    rc, msg = _call(entry, row_tags=None, query_masks=None, tag_match=77)
    assert rc == WORKSPACE and "workspace" in msg, (rc, msg)
    rc, msg = _call(entry, row_tags=None, query_masks=None, tag_match=77, k=257)        # ... and says so in its refusals
    assert rc == UNSUPPORTED and msg.startswith(base), (rc, msg)
    if entry == "tagged":
        for algo in (QUERY, BUCKET):
            rc, msg = _call(entry, row_tags=None, query_masks=None, row_filter=None, algo=algo)
            assert rc == WORKSPACE and "workspace" in msg, (rc, msg)
            rc, msg = _call(entry, row_tags=None, query_masks=None, row_filter=None, algo=algo, k=65)
            assert rc == UNSUPPORTED and msg.startswith("scan_topk_typed:"), (rc, msg)
    # an empty batch is valid without its pointers
    nulls = {name: None for name, value in TAG_VALID.items() if value == FAKE and name in ENTRIES[entry][1]}
    rc, msg = _call(entry, Q=0, **nulls)
    assert rc == OK, (rc, msg)


def test_the_step_and_graph_paths_refuse_tags_in_the_one_check():
    """The internal paths (`NLSH_PHASE_PLAN_REST`, graph nodes) have no parameter for tags; the refusals that guard them are in the
    sources of the one check and of the node builder, next to the row filter's."""
    import os
    csrc = os.path.join(os.path.dirname(_capi.CSRC), "csrc")
    check = open(os.path.join(csrc, "scan_topk.hip")).read()
    assert "row_tags are read by the direct top-k calls only" in check and "SCAN_ALLOWS_PLAN_REST" in check
    node = open(os.path.join(csrc, "scan_bucket.hip")).read()
    assert "a call with row_tags cannot be replayed from a graph node" in node


# ---------------------------------------------------------------------------------------------- facade refusals
def _bare_indexer(metric="l2", tags=True):
    from nlsh_amd.indexer import Indexer
    ix = Indexer.__new__(Indexer)           # the validation below runs before the index's arrays are touched
    ix.metric, ix.algo, ix.generation = metric, None, 0
    if tags:
        ix.tags_sorted = torch.zeros(5, dtype=torch.int64)
    return ix


class _Q:
    shape = (4, 8)


def test_facade_refusals_before_any_launch():
    from nlsh_amd.indexer import Indexer, TagFilter
    ix = _bare_indexer()
    f = ix._checked_filter(None, None, 5, "all", _Q)
    assert isinstance(f, TagFilter) and (f.mask, f.match, f.row_filter) == (5, _capi.TAG_ALL, None)
    assert ix._checked_filter(f) is f                                   # handed on between the calls of the class
    assert ix._checked_filter(None, None, (1 << 64) - 1, "any", _Q).mask == -1 and ix._checked_filter(None, None, 1 << 63, "eq", _Q).mask == -(1 << 63)
    t = torch.zeros(4, dtype=torch.int64)
    assert ix._checked_filter(None, None, t, "eq", _Q).mask is t
    with pytest.raises(ValueError, match="built without tags"):
        _bare_indexer(tags=False)._checked_filter(None, None, 1, "any", _Q)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int64),
                torch.zeros(4, dtype=torch.float32), 1.5, True, "7", [1, 2, 3, 4]):
        with pytest.raises(ValueError, match="tag_mask must be"):
            ix._checked_filter(None, None, bad, "any", _Q)
    for bad in (1 << 64, -(1 << 63) - 1):
        with pytest.raises(ValueError, match="64 bits"):
            ix._checked_filter(None, None, bad, "any", _Q)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="tag_mask is on"):
            ix._checked_filter(None, None, t.cuda(), "any", _Q)
    for bad in ("some", None, 0, "ANY"):
        with pytest.raises(ValueError, match="tag_match"):
            ix._checked_filter(None, None, 1, bad, _Q)
    for forced in ("query", "bucket"):
        ix.algo = forced
        with pytest.raises(ValueError, match="tiled"):
            ix._checked_filter(None, None, 1, "any", _Q)
    ix.algo = "tiled"
    with pytest.raises(ValueError, match="tiled"):
        ix._checked_filter(None, _capi.SCAN_BUCKET_MAJOR, 1, "any", _Q)
    with pytest.raises(NotImplementedError, match="tag_mask"):
        _bare_indexer("generic")._checked_filter(None, None, 1, "any", _Q)
    # the public calls check first: nothing of the (absent) index arrays is touched before the refusal
    plain = _bare_indexer(tags=False)
    for call in (lambda: plain.query(_Q, tag_mask=1), lambda: plain.query_tensors(_Q, tag_mask=1),
                 lambda: plain.scan_tensors(_Q, None, None, tag_mask=1), lambda: plain.query_with_keys(_Q, [], tag_mask=1)):
        with pytest.raises(ValueError, match="built without tags"):
            call()
    # out of scope: named refusals
    for call in (lambda: ix.range_scan_tensors(None, None, None, 1.0, tag_mask=1), lambda: ix.range_tensors(None, 1.0, tag_mask=1),
                 lambda: ix.range_query(None, 1.0, tag_mask=1), lambda: ix.range_query_with_keys(None, [], 1.0, tag_mask=1)):
        with pytest.raises(NotImplementedError, match="tag_mask"):
            call()
    from nlsh_amd.distributed import ShardedIndexer
    from nlsh_amd.pipeline import QueryPipeline
    with pytest.raises(NotImplementedError, match="tag_mask"):
        QueryPipeline(ix, None, tag_mask=1)
    with pytest.raises(NotImplementedError, match="tag_mask"):
        ShardedIndexer(None, None, None, id_base=0, tags=torch.zeros(3, dtype=torch.int64))
    sh = ShardedIndexer.__new__(ShardedIndexer)
    for call in (lambda: sh.query_tensors(None, tag_mask=1), lambda: sh.query(None, tag_mask=1)):
        with pytest.raises(NotImplementedError, match="tag_mask"):
            call()
    # tags of the constructor, add and set_tags
    host = torch.zeros((6, 4))
    for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros(6, dtype=torch.int32), [0] * 6, torch.zeros((6, 1), dtype=torch.int64)):
        with pytest.raises(ValueError, match="tags must be an int64 tensor"):
            Indexer(None, host, None, metric="l2", tags=bad)
    with pytest.raises(ValueError, match="built without tags"):
        plain.update(add=host, add_tags=torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ValueError, match="built without tags"):
        plain.add(host, tags=torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ValueError, match="built without tags"):
        plain.set_tags([1], torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="built without tags"):
        plain.tags_local()


# ---------------------------------------------------------------------------------------------- the generator is not vacuous
def _host_world(monkeypatch):
    """`_world("float16")` of tests/test_gpu_row_filter.py with its tensors left on the host (and its cache left alone)."""
    import test_gpu_row_filter as rf
    monkeypatch.setattr(rf, "_worlds", {})
    monkeypatch.setattr(rf, "dev", lambda x: torch.from_numpy(np.ascontiguousarray(x)))
    return rf._world("float16")


def test_the_generator_covers_full_short_and_empty_lists_in_every_group(monkeypatch):
    w = _host_world(monkeypatch)
    N, Q = len(w["ids"]), w["Q"]
    assert 9000 < N < 10500 and Q == 72 and w["S"].shape[1] == 100
    masks = ref.query_masks(Q)
    assert len(set(masks.tolist())) == 7 and masks[:7].tolist() == ref.MASKS.tolist()
    forced = w["rows_of"][ref.forced_bucket(w["buckets"])]
    kh, nh = w["keys"].numpy(), w["nkeys"].numpy()
    bucket_of_key = {int(w["corpus_keys"][rows[0]]): b for b, rows in w["rows_of"].items()}
    cands = [np.concatenate([w["rows_of"][bucket_of_key[int(key)]] for key in kh[qi, :nh[qi]] if int(key) in bucket_of_key] or [np.zeros(0, np.int64)])
             for qi in range(Q)]
    short = empty = False
    for mode in ref.MODES:
        tags = ref.tags_for(mode, N, forced)
        assert tags.dtype == U64 and (tags == 0).sum() >= ref.N_FORCED and (tags == ref.ALL_ONES).sum() >= ref.N_FORCED
        if mode != "eq":
            assert not ((tags >> U64(ref.RESERVED_BIT)) & U64(1))[tags != ref.ALL_ONES].any()
            dens = np.asarray([bin(int(t)).count("1") for t in tags])
            assert (dens < 8).sum() > N // 8 and (dens > 50).sum() > N // 8                 # mixed densities
        else:
            assert set(tags.tolist()) == set(ref.LABELS.tolist())
        for mi, mask in enumerate(ref.MASKS):
            counts = [int(ref.passes(tags[cands[qi]], mask, mode).sum()) for qi in range(Q) if qi % 7 == mi]
            whole = int(ref.passes(tags, mask, mode).sum())
            if (mode, mi) in ref.EMPTY_GROUPS:
                assert whole == 0, (mode, mi)
            else:
                assert max(counts) >= 10, (mode, mi, counts)
            if mode == "all" and mi in (1, 6):      # passed by the forced ~0 rows alone
                assert whole == ref.N_FORCED, (mi, whole)
            short |= any(1 <= c <= 9 for c in counts)
            empty |= any(c == 0 for c in counts)
    assert short and empty
    # one 16-query group of one bucket with >= 4 distinct masks: a bucket probed by exactly 16 queries is one group
    prober = {b: [qi for qi in range(Q) if any(bucket_of_key.get(int(key)) == b for key in kh[qi, :nh[qi]])] for b in w["rows_of"]}
    assert any(len(qs) == 16 and len({qi % 7 for qi in qs}) >= 4 for b, qs in prober.items() if w["buckets"][b][1] == 16)
