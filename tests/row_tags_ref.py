"""Per-query tag filters: the pass rule in numpy on uint64 words, and the generator of the tags and masks the tests use.

A row carries a 64-bit tag, a query a 64-bit mask, a call one mode: "any" -- (tag & mask) != 0; "all" -- (tag & mask) == mask;
"eq" -- tag == mask.  The project keeps both in int64 tensors and reads the bits as unsigned; here they are uint64 throughout and
`as_i64` reinterprets.

The seven masks, dealt to the queries round-robin (mask[i] = MASKS[i % 7]): 0, ~0, one low bit, one bit in each 32-bit half, bit 63, three
bits across the halves, and RESERVED -- two bits of which one (bit 47) no generated tag carries.

Tags: `tags_bits` (modes "any" and "all") draws every row's bits at one of four densities, never bit 47, and forces rows of 0 and of
~0; `tags_labels` (mode "eq") draws every row one of six labels -- the first six masks, 0 and a value with bit 63 among them.

What passes nothing, by construction: ("any", 0) and ("eq", RESERVED).  Under "all" the mask RESERVED is passed by the forced ~0 rows
and by no other row (a tag of ~0 passes every "all" mask, so "no row at all" and "forced rows of ~0" cannot both hold; the forced rows sit
in ONE bucket, and every query that does not probe it gets an all-padding list from this mask), and so is the mask ~0."""
import numpy as np

U64 = np.uint64
ALL_ONES = U64(0xFFFFFFFFFFFFFFFF)
LOW, HALVES, BIT63 = U64(1 << 3), U64((1 << 5) | (1 << 40)), U64(1 << 63)
THREE = U64((1 << 1) | (1 << 33) | (1 << 62))
RESERVED_BIT = 47
RESERVED = U64((1 << RESERVED_BIT) | (1 << 13))
MASKS = np.asarray([0, ALL_ONES, LOW, HALVES, BIT63, THREE, RESERVED], dtype=U64)
LABELS = MASKS[:6]
MODES = ("any", "all", "eq")
EMPTY_GROUPS = {("any", 0), ("eq", 6)}      # (mode, index into MASKS) that no row passes, whatever the tags drawn below
N_FORCED = 12                               # rows of ~0 (and as many of 0) forced into one bucket


def passes(tags, mask, mode):
    """bool array: which of `tags` (uint64 array) pass `mask` (one uint64, or an array that broadcasts) under `mode`."""
    tags, mask = np.asarray(tags, dtype=U64), np.asarray(mask, dtype=U64)
    both = tags & mask
    if mode == "any":
        return both != U64(0)
    if mode == "all":
        return both == mask
    if mode == "eq":
        return tags == mask
    raise ValueError(mode)


def as_i64(words):
    """The same 64 bits in the signed container the project's tensors use."""
    return np.ascontiguousarray(np.asarray(words, dtype=U64)).view(np.int64)


def query_masks(Q):
    return MASKS[np.arange(Q) % len(MASKS)]


def tags_bits(N, forced_rows, seed=5):
    """uint64 [N]: per row a density in {0.05, 0.3, 0.6, 0.9}, each bit but RESERVED_BIT set with it; `forced_rows` (>= 2 * N_FORCED local
    rows of one bucket): the first N_FORCED become 0, the next N_FORCED ~0."""
    rng = np.random.default_rng(seed)
    density = np.asarray([0.05, 0.3, 0.6, 0.9])[rng.integers(0, 4, size=N)]
    bits = rng.random((N, 64)) < density[:, None]
    bits[:, RESERVED_BIT] = False
    tags = (bits.astype(U64) << np.arange(64, dtype=U64)[None, :]).sum(axis=1, dtype=U64)
    forced_rows = np.asarray(forced_rows)
    assert len(forced_rows) >= 2 * N_FORCED
    tags[forced_rows[:N_FORCED]] = U64(0)
    tags[forced_rows[N_FORCED:2 * N_FORCED]] = ALL_ONES
    return tags


def tags_labels(N, forced_rows, seed=6):
    """uint64 [N]: one of the six LABELS per row; the forced rows as in `tags_bits` (0 and ~0 are labels)."""
    rng = np.random.default_rng(seed)
    tags = LABELS[rng.integers(0, len(LABELS), size=N)].copy()
    forced_rows = np.asarray(forced_rows)
    tags[forced_rows[:N_FORCED]] = U64(0)
    tags[forced_rows[N_FORCED:2 * N_FORCED]] = ALL_ONES
    return tags


def tags_for(mode, N, forced_rows):
    return tags_labels(N, forced_rows) if mode == "eq" else tags_bits(N, forced_rows)


def forced_bucket(buckets):
    """The bucket the forced rows sit in: the 700-row bucket probed by 17 queries (three segments, two query groups)."""
    return next(b for b, (s, m) in enumerate(buckets) if s == 700 and m == 17)
