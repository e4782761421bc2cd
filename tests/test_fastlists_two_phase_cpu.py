"""CPU-only: the two-phase list construction of csrc/fastlists.c (`rows_alloc` -- the containers, `rows_fill` -- a row range's ids and
counts) builds what `ndarray.tolist()` builds, keeps its unfilled lists where nothing can find them, refuses what it cannot fill
before storing anything, and releases a shell that is dropped at any stage."""
import gc
import sys

import numpy as np
import pytest

from nlsh_amd import indexer

SHAPES = ((0, 10), (1, 1), (257, 10), (1000, 64))


def _helper():
    assert indexer._rows_alloc is not None and indexer._rows_fill is not None, "csrc/fastlists.c was not built (make -C csrc)"
    return indexer._rows_alloc, indexer._rows_fill


def _block(shape, seed=5):
    rng = np.random.default_rng(seed)
    a = rng.integers(-1, 2 ** 31 - 1, size=shape, endpoint=True).astype(np.int32)
    if a.size:
        a.flat[0], a.flat[-1] = -1, 2 ** 31 - 1           # both ends of the id range are present whatever the draw
    return a, rng.integers(0, 2 ** 31 - 1, size=shape[0], endpoint=True).astype(np.int32)


def _ranges(Q, parts, reverse):
    bounds = [(Q * c // parts, Q * (c + 1) // parts) for c in range(parts)]
    return bounds[::-1] if reverse else bounds


@pytest.mark.parametrize("reverse", (False, True))
@pytest.mark.parametrize("parts", (1, 2, 3))
@pytest.mark.parametrize("shape", SHAPES)
def test_two_phase_lists_are_ndarray_tolist(shape, parts, reverse):
    alloc, fill = _helper()
    Q, k = shape
    a, nc = _block(shape)
    for untrack in (False, True):
        outer, counts = alloc(Q, k), [0] * Q
        for lo, hi in _ranges(Q, parts, reverse):
            if untrack:
                fill(outer, lo, hi, a[lo:hi], nc[lo:hi], counts, True)
            else:
                fill(outer, lo, hi, a[lo:hi], nc[lo:hi], counts)
        assert outer == a.tolist() and counts == nc.tolist()
        assert type(outer) is list and all(type(row) is list for row in outer)
        assert all(type(v) is int for row in outer for v in row) and all(type(c) is int for c in counts)
        assert gc.is_tracked(outer)
        assert all(gc.is_tracked(row) != untrack for row in outer)


def test_unfilled_rows_are_invisible_to_the_collector():
    """Neither the shell nor a row of it is on the collector before its fill: `gc.get_objects()` returns no half-built list, and the
    outer list appears with the fill that completes it."""
    alloc, fill = _helper()
    Q, k = 300, 7
    a, nc = _block((Q, k))
    outer, counts = alloc(Q, k), [0] * Q
    # identities taken from a collector snapshot, never by indexing the shell: an unfilled row must not be handed to Python code
    def tracked_ids():
        return {id(o) for o in gc.get_objects()}
    assert not gc.is_tracked(outer) and id(outer) not in tracked_ids()
    fill(outer, 100, 200, a[100:200], nc[100:200], counts)
    seen = tracked_ids()
    assert not gc.is_tracked(outer) and id(outer) not in seen
    filled = outer[100:200]
    assert all(id(row) in seen for row in filled) and filled == a[100:200].tolist()
    # every list the collector knows can be read element by element (an empty slot would be a NULL handed to the interpreter)
    assert all(v is not NotImplemented for o in gc.get_objects() if type(o) is list and len(o) == k for v in o)
    fill(outer, 200, Q, a[200:], nc[200:], counts)
    assert not gc.is_tracked(outer)
    fill(outer, 0, 100, a[:100], nc[:100], counts)
    assert gc.is_tracked(outer) and id(outer) in tracked_ids() and outer == a.tolist() and counts == nc.tolist()
    gc.collect()                        # a full collection walks the finished lists like any others
    assert outer == a.tolist()


def test_refusals_store_nothing():
    alloc, fill = _helper()
    Q, k = 12, 5
    a, nc = _block((Q, k))
    outer, counts = alloc(Q, k), [0] * Q

    def refused(*args):
        with pytest.raises(ValueError):
            fill(*args)
        assert counts == [0] * Q and not gc.is_tracked(outer)

    refused(outer, 0, Q, a[:Q - 1], nc, counts)                       # a short ids block
    refused(outer, 0, Q, a, nc[:Q - 1], counts)                       # a short counts block
    refused(outer, 5, 4, a[:0], nc[:0], counts)                       # lo > hi
    refused(outer, 0, Q + 1, np.zeros((Q + 1, k), np.int32), np.zeros((Q + 1,), np.int32), counts)    # hi > Q
    refused(outer, -1, 3, a[:4], nc[:4], counts)
    refused(outer, 0, Q, np.zeros((Q, k + 1), np.int32), nc, counts)  # rows of another length than the ids'
    refused(outer, 0, Q, np.zeros((Q, k - 1), np.int32), nc, counts)
    refused(outer, 0, Q, a.astype(np.int64), nc, counts)              # not int32
    refused(outer, 0, Q, a.reshape(-1), nc, counts)                   # not [hi - lo, k]
    refused(outer, 0, Q, a, nc, [0] * (Q - 1))                        # counts_out of another length
    with pytest.raises((ValueError, BufferError)):
        fill(outer, 0, Q // 2, a[::2], nc[::2], counts)               # not C-contiguous
    assert counts == [0] * Q
    # everything above stored nothing: the whole shell is still fillable, in two ranges ...
    fill(outer, 0, 6, a[:6], nc[:6], counts)
    # ... a second fill of the same range, or of one that overlaps it by a row, is refused and changes nothing
    before = counts[:]
    for lo, hi in ((0, 6), (5, Q), (0, Q)):
        with pytest.raises(ValueError):
            fill(outer, lo, hi, np.zeros((hi - lo, k), np.int32), np.zeros((hi - lo,), np.int32), counts)
    assert counts == before and outer[:6] == a[:6].tolist()
    fill(outer, 6, Q, a[6:], nc[6:], counts)
    assert outer == a.tolist() and counts == nc.tolist() and gc.is_tracked(outer)
    # a list of ordinary lists is "already filled"; a list of other things is not a shell
    with pytest.raises(ValueError):
        fill([[1] * k for _ in range(Q)], 0, Q, a, nc, [0] * Q)
    with pytest.raises(ValueError):
        fill([None] * Q, 0, Q, a, nc, [0] * Q)
    with pytest.raises(ValueError):
        alloc(-1, 3)


def test_short_rows_replaced_between_fills():
    """The facade replaces the rows of short queries right after their range's fill, before later ranges are filled: a replaced row
    (any list, of any length) counts as filled."""
    alloc, fill = _helper()
    Q, k = 9, 4
    a, nc = _block((Q, k))
    outer, counts = alloc(Q, k), [0] * Q
    fill(outer, 0, 4, a[:4], nc[:4], counts)
    outer[1], outer[3] = [], [7, 8, 9, 10, 11, 12]
    fill(outer, 4, Q, a[4:], nc[4:], counts)
    want = a.tolist()
    want[1], want[3] = [], [7, 8, 9, 10, 11, 12]
    assert outer == want and gc.is_tracked(outer) and counts == nc.tolist()


def _settled_blocks(fn, rounds=200):
    fn()
    fn()
    gc.collect()
    start = sys.getallocatedblocks()
    for _ in range(rounds):
        fn()
    gc.collect()
    return sys.getallocatedblocks() - start


def test_dropped_shells_release_everything():
    """An unfilled shell, a half-filled one and a finished one, each built and dropped 200 times: the allocator's block count ends
    within a small constant of where it started (one leaked row per round would be 200 blocks, one leaked int per row 10^4)."""
    alloc, fill = _helper()
    Q, k = 64, 10
    a, nc = _block((Q, k))

    def unfilled():
        alloc(Q, k)

    def half():
        outer, counts = alloc(Q, k), [0] * Q
        fill(outer, 16, 48, a[16:48], nc[16:48], counts)

    def full():
        outer, counts = alloc(Q, k), [0] * Q
        fill(outer, 0, 32, a[:32], nc[:32], counts)
        fill(outer, 32, Q, a[32:], nc[32:], counts, True)

    def refused():
        outer, counts = alloc(Q, k), [0] * Q
        with pytest.raises(ValueError):
            fill(outer, 0, Q, a[:5], nc, counts)

    for fn in (unfilled, half, full, refused):
        assert abs(_settled_blocks(fn)) <= 16, fn.__name__


def test_plain_lists_is_still_tolist():
    idx, nc = np.arange(5120, dtype=np.int32).reshape(512, 10), np.full((512,), 12, dtype=np.int32)
    lists, counts = indexer.Indexer._plain_lists(idx, nc)
    assert lists == idx.tolist() and counts == nc.tolist()
    assert all(type(row) is list for row in lists) and all(gc.is_tracked(row) for row in lists)
