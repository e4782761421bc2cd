"""Mass-tie data and the high-precision reference of the (distance, global row id) order -- numpy only, no GPU, no project kernel.

A tie corpus holds nothing but exact copies of a dozen prototype vectors, so a query has at most a dozen distinct distances and every
one of them is shared by up to thousands of rows, scattered over buckets, segments, tasks, cell windows and shards.  The expected top-k
is then a statement about PROTOTYPES -- sort the candidates by (fp64 distance of the row's prototype, global id) -- which is unambiguous
as long as two prototypes never come closer to a query than the schedules' distance tolerance can move them: `separation` measures that
and the CPU test holds every data set to SEPARATION (tests/test_tie_order_cpu.py).  Nothing here ever looks at a device distance."""
import functools
from types import SimpleNamespace

import numpy as np

from helpers import fp64_distances

KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
DIST_RTOL = 2e-5          # every schedule: |d_hip - d_fp64| <= 2e-5 * max(1, |d|) (parity bars)
SEPARATION = 1e-4         # two prototypes swap only when closer than 2 * DIST_RTOL = 4e-5: 2.5x over that
NARROW_K = (1, 10, 32, 33, 64)
WIDE_K = (65, 128, 129, 192, 193, 256)
ALL_K = NARROW_K + WIDE_K
N_QUERIES = 48
N_BIG_GROUPS = 8
SMALL_GROUPS = (1, 2, 3, 9)                                # multiplicities of prototypes 8..11
DIM = {"l2": 24, "cosine": 25}                             # cosine: d % 4 != 0, the prepared-query path
SEED = 11                                                  # a seed for which SEPARATION holds at both dimensions (the CPU test asserts it)


# ----------------------------------------------------------------------------- sort keys (csrc/common.h restated)
def mono_from_float(f):
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def float_from_mono(m):
    m = np.ascontiguousarray(m, dtype=np.uint32)
    return np.where(m & np.uint32(0x80000000), m & np.uint32(0x7FFFFFFF), ~m).astype(np.uint32).view(np.float32)


def make_keys(dist, ids):
    """uint64 sort keys monotone(dist) << 32 | id, as the kernels pack them."""
    return (mono_from_float(dist).astype(np.uint64) << np.uint64(32)) | (np.asarray(ids, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF))


def merge_reference(keys_in, k):
    """nlsh_merge_topk restated: keys_in uint64 [G, Q, row_stride >= k]; per query the first k keys of the G lists, ~0 dropped, sorted
    as uint64, the first k -> (dist fp32 [Q, k] +inf padded, idx int32 [Q, k] -1 padded)."""
    keys_in = np.asarray(keys_in, dtype=np.uint64)
    G, Q, _ = keys_in.shape
    dist = np.full((Q, k), np.inf, dtype=np.float32)
    idx = np.full((Q, k), -1, dtype=np.int32)
    for q in range(Q):
        keys = keys_in[:, q, :k].reshape(-1)
        keys = np.sort(keys[keys != KEY_NONE])[:k]
        dist[q, :len(keys)] = float_from_mono((keys >> np.uint64(32)).astype(np.uint32))
        idx[q, :len(keys)] = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    return dist, idx


# ----------------------------------------------------------------------------- data
def tie_corpus(metric, d, layout, seed):
    """layout: one (corpus key, {prototype: rows}) per bucket.  -> corpus fp32 [N, d] (every row an exact copy of a prototype),
    corpus_keys int32 [N], group_of_row int32 [N], prototypes fp32 [G, d].  Rows are placed by a seeded permutation: the ids of a tie
    group are scattered over the buckets and over the positions inside a bucket."""
    assert metric in DIM
    rng = np.random.default_rng(seed)
    n_groups = 1 + max(g for _, comp in layout for g in comp)
    prototypes = rng.standard_normal((n_groups, d)).astype(np.float32)
    key_of_slot = np.concatenate([np.full(sum(comp.values()), key, np.int32) for key, comp in layout])
    group_of_slot = np.concatenate([np.full(n, g, np.int32) for _, comp in layout for g, n in sorted(comp.items())])
    N = len(key_of_slot)
    row_of_slot = rng.permutation(N)
    corpus_keys, group_of_row = np.empty(N, np.int32), np.empty(N, np.int32)
    corpus_keys[row_of_slot], group_of_row[row_of_slot] = key_of_slot, group_of_slot
    return prototypes[group_of_row].copy(), corpus_keys, group_of_row, prototypes


def tie_queries(d, seed, n=N_QUERIES):
    return np.random.default_rng([seed, 0x71]).standard_normal((n, d)).astype(np.float32)


def prototype_distances(queries, prototypes, metric):
    """fp64 [Q, G]: helpers.fp64_distances of every query to every prototype."""
    return np.stack([fp64_distances(q, prototypes, metric) for q in queries])


def separation(queries, prototypes, metric):
    """min over ALL queries and consecutive distinct prototype distances of gap / max(1, |d|) (no query is skipped)."""
    worst = np.inf
    for row in prototype_distances(queries, prototypes, metric):
        s = np.unique(row)
        if len(s) > 1:
            worst = min(worst, float((np.diff(s) / np.maximum(1.0, np.maximum(np.abs(s[1:]), np.abs(s[:-1])))).min()))
    return worst


def candidate_rows(corpus_keys, key_lists):
    """Rows (ascending) of every query's probed buckets; a repeated key probes its bucket once, an unknown key none."""
    return [np.nonzero(np.isin(corpus_keys, np.asarray(sorted(set(int(v) for v in ks)), dtype=np.int64)))[0] for ks in key_lists]


def expected_topk(queries, prototypes, group_of_row, ids, candidate_rows, k, metric):
    """The reference: candidates sorted by (fp64 distance of the row's PROTOTYPE, global id), first k.
    ids [N]: global id of every row; candidate_rows: per query the rows (indices into group_of_row / ids) of its probed buckets.
    -> idx int32 [Q, k] (-1 padded), d64 [Q, k] (+inf padded), ncand int64 [Q]."""
    pd = prototype_distances(queries, prototypes, metric)
    Q = len(queries)
    idx = np.full((Q, k), -1, dtype=np.int32)
    d64 = np.full((Q, k), np.inf, dtype=np.float64)
    ncand = np.zeros(Q, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    for q in range(Q):
        rows = np.asarray(candidate_rows[q], dtype=np.int64)
        ncand[q] = len(rows)
        dd, gid = pd[q, group_of_row[rows]], ids[rows]
        order = np.lexsort((gid, dd))[:k]
        idx[q, :len(order)], d64[q, :len(order)] = gid[order], dd[order]
    return idx, d64, ncand


def cut_classes(pd_row, groups_of_candidates, k):
    """Which kinds of cut one query's candidate set is, from the reference alone: "short" (< k candidates), "exact" (== k), "inside"
    (the k-th place falls strictly inside a tie group: select_k_smallest's c_eq > need), "group_end" (more than k candidates and the
    cut is exactly at a group's end), "one_group" (all candidates are copies of one prototype)."""
    n = len(groups_of_candidates)
    out = set()
    groups, counts = np.unique(groups_of_candidates, return_counts=True)
    if n and len(groups) == 1:
        out.add("one_group")
    if n < k:
        out.add("short")
    elif n == k:
        out.add("exact")
    else:
        ends = np.cumsum(counts[np.argsort(pd_row[groups], kind="stable")])
        out.add("group_end" if k in ends.tolist() else "inside")
    return out


def list_counts(bucket_rows, key_lists, seg):
    """Per query (L, widest probe): the merge's partial lists sum(ceil(bucket rows / seg)) and the most segments of one probe."""
    out = []
    for ks in key_lists:
        segs = [-(-bucket_rows[int(v)] // seg) for v in dict.fromkeys(ks) if int(v) in bucket_rows]
        out.append((sum(segs), max(segs + [0])))
    return out


def merge_classes(L, widest, k):
    """The forms of merge_query (csrc/scan_bucket_merge.h) one query takes at k <= 64: R = 64 // k lists per load."""
    R = 64 // k
    out = {"le_R" if L <= R else "le_2R" if L <= 2 * R else "one_round" if L <= 3 * R else "rounds"}
    if L > 128:
        out.add("gt_128")
    if widest > 8:
        out.add("probe_gt_8")
    return out


# ----------------------------------------------------------------------------- layouts
BIG = {10: 64, 20: 256, 30: 700, 40: 2100}                    # key -> rows; 2100 rows: 9 tiled segments, the untabbed list search
SMALL_KEY0, EDGE_KEY0, UNKNOWN_KEY = 1000, 2000, 7777


def _mixed(rng, rows, groups=N_BIG_GROUPS):
    p = rng.dirichlet(np.full(groups, 0.7))
    counts = rng.multinomial(rows, p)
    return {g: int(n) for g, n in enumerate(counts) if n}


def _plant(comp, group):
    """One row of the bucket's most frequent prototype becomes a row of `group` (the bucket keeps its size)."""
    top = max(comp, key=lambda g: (comp[g], -g))
    assert comp[top] > 1
    comp[top] -= 1
    comp[group] = comp.get(group, 0) + 1


def main_layout(seed=0):
    """Buckets of 64 / 256 / 700 / 2100 rows, 40 consecutive buckets of 1..20 rows (they share cell windows; those of <= 3 rows hold one
    prototype), and per k of ALL_K an edge bucket {a: k, b: k}: probed alone it has 2 k candidates and, whichever of a and b is nearer to
    the query, the cut is exactly at that group's end; probed at a larger k' < 2 k it is strictly inside the farther group.  Prototypes
    8..11 are the small tie groups of 1, 2, 3 and 9 rows."""
    rng = np.random.default_rng([seed, 0x1a])
    layout = [(key, _mixed(rng, rows)) for key, rows in BIG.items()]
    sizes = np.concatenate([rng.permutation(20) + 1, rng.permutation(20) + 1])
    for i, rows in enumerate(sizes.tolist()):
        layout.append((SMALL_KEY0 + i, {int(rng.integers(N_BIG_GROUPS)): rows} if rows <= 3 else _mixed(rng, rows, 4)))
    for i, k in enumerate(ALL_K):
        layout.append((EDGE_KEY0 + i, {i % N_BIG_GROUPS: k, (i + 3) % N_BIG_GROUPS: k}))
    small = [b for b in range(4, 44) if sum(layout[b][1].values()) >= 10]
    homes = {8: [3], 9: [2, small[0]], 10: [0, 1, small[1]], 11: [3, 3, 3, 1, 1, 1, small[2], small[3], small[4]]}
    for group, buckets in homes.items():
        assert len(buckets) == SMALL_GROUPS[group - N_BIG_GROUPS]
        for b in buckets:
            _plant(layout[b][1], group)
    return layout


LISTS_SMALL = {50: 40, 60: 100}                               # 1 and 2 lists of 64 rows
LISTS_MID_KEY0, LISTS_N_MID = 3000, 45                        # 45 buckets of 150..190 rows: 3 lists each
LISTS_BIG = {9000: 2100, 9001: 2100}                          # 33 lists each: a probe of more than 8 segments


def lists_layout(seed=0):
    """The layout of the seg_rows = 64 merges: per-query list counts from 1 to 204 (more than 128: the untabbed search; more than
    3 * 64: several rounds even at k = 1)."""
    rng = np.random.default_rng([seed, 0x2b])
    layout = [(key, _mixed(rng, rows)) for key, rows in LISTS_SMALL.items()]
    layout += [(LISTS_MID_KEY0 + i, _mixed(rng, int(rng.integers(150, 191)))) for i in range(LISTS_N_MID)]
    layout += [(key, _mixed(rng, rows)) for key, rows in LISTS_BIG.items()]
    for group, n in zip(range(N_BIG_GROUPS, N_BIG_GROUPS + 4), SMALL_GROUPS):
        for b in rng.choice(len(layout), size=n, replace=True).tolist():
            _plant(layout[b][1], group)
    return layout


def one_layout():
    """An all-identical corpus: one prototype, ~3000 rows -- every distance of every query ties."""
    return [(10, {0: 64}), (20, {0: 700}), (30, {0: 2100})] + [(SMALL_KEY0 + i, {0: 1 + i % 20}) for i in range(12)]


def _subset_with_total(bucket_rows, total, max_keys=60):
    """Keys of distinct buckets whose rows add up to `total` (smallest buckets first), or None."""
    best = {0: []}
    for key, rows in sorted(bucket_rows.items(), key=lambda kv: kv[1]):
        for t, ks in sorted(best.items(), reverse=True):
            if t + rows <= total and t + rows not in best and len(ks) < max_keys:
                best[t + rows] = ks + [key]
    return best.get(total)


def main_key_lists(bucket_rows, k):
    """48 key lists on main_layout for one k: single buckets (every size class, the k's edge bucket), a few buckets, all of them, sets
    with exactly k and k - 1 candidates, an unknown key, none, a repeated key, different small buckets of one window."""
    plain = {key: rows for key, rows in bucket_rows.items() if key < EDGE_KEY0}
    small = sorted(key for key in bucket_rows if SMALL_KEY0 <= key < EDGE_KEY0)
    edge = EDGE_KEY0 + ALL_K.index(k)
    edge2 = EDGE_KEY0 + (ALL_K.index(k) + 1) % len(ALL_K)                        # the next k's: 2 k' candidates
    edges = sorted(key for key in bucket_rows if key >= EDGE_KEY0)
    every = sorted(bucket_rows)                                                   # 55 buckets: P <= 64
    pure = [key for key in small if bucket_rows[key] <= 3]
    exact, short = _subset_with_total(plain, k), _subset_with_total(plain, k - 1)
    assert exact is not None and short is not None
    lists = [
        [10], [20], [30], [40], [edge], [edge2], [edge, edge2], [edge2, edge],
        every, every[::-1], every, every,
        exact, exact[::-1], short, short + [UNKNOWN_KEY],
        [UNKNOWN_KEY], [], [40, 40, 30, 40], [pure[0]],
        [40, edge2], [30, 20, 10], [10] + small[:8], small,
        small[:10], small[5:15], small[10:20], small[20:], small[::2], small[1::2], [small[3]], [small[4], small[5]],
        [40, 30] + small, [20, edge] + small[:5], [30, UNKNOWN_KEY, 40], [pure[1], pure[2]],
        edges, [EDGE_KEY0, EDGE_KEY0 + 5, EDGE_KEY0 + 10], [10, 20], [40, 20],
        every, every[5:], every[:40], [30, edge],
        [edge, 10], small[30:] + [40], [20] + small[15:25], every[::3],
    ]
    assert len(lists) == N_QUERIES and max(len(ks) for ks in lists) <= 64
    return lists


def lists_key_lists(bucket_rows):
    """48 key lists on lists_layout: list counts (at 64 rows per list) 1, 2, 3, 4, 5, 6, 7, 12, 13, 18, 21, ... 90, 135, 204."""
    a, b = sorted(LISTS_SMALL)
    mid = [LISTS_MID_KEY0 + i for i in range(LISTS_N_MID)]
    big = sorted(LISTS_BIG)
    every = [a, b] + mid + big
    base = [
        [a], [b], [a, b], mid[:1], [a] + mid[:1], [b] + mid[:1], mid[:2], [a] + mid[:2],
        mid[:4], [a] + mid[:4], mid[:6], mid[:7], mid[:30], mid, every, every[::-1],
        big[:1], big, [a] + big[:1], mid[:21], mid[10:], [b] + mid[40:], [UNKNOWN_KEY], mid[::-1],
    ]
    lists = base + [ks[::-1] for ks in base]
    assert len(lists) == N_QUERIES and max(len(ks) for ks in lists) <= 64
    return lists


def one_key_lists():
    every = [10, 20, 30] + [SMALL_KEY0 + i for i in range(12)]
    base = [[10], [20], [30], every, every[::-1], [SMALL_KEY0], [SMALL_KEY0 + 1, SMALL_KEY0 + 2], every[3:],
            [30, 10], [UNKNOWN_KEY], [20, SMALL_KEY0 + 9], every[::2]]
    return base * 4


@functools.lru_cache(maxsize=None)
def dataset(metric, name):
    """One data set of the tie tests ("main" | "lists" | "one") -- the CPU test holds each to SEPARATION and the coverage classes, the
    GPU tests run the kernels on it."""
    layout = {"main": main_layout, "lists": lists_layout, "one": one_layout}[name]()
    d, seed = DIM[metric], SEED
    corpus, corpus_keys, group_of_row, prototypes = tie_corpus(metric, d, layout, seed)
    bucket_rows = {int(key): sum(comp.values()) for key, comp in layout}
    return SimpleNamespace(metric=metric, name=name, d=d, layout=layout, corpus=corpus, corpus_keys=corpus_keys, group_of_row=group_of_row,
                           prototypes=prototypes, queries=tie_queries(d, seed), bucket_rows=bucket_rows, N=len(corpus))


def key_lists_of(data, k):
    if data.name == "main":
        return main_key_lists(data.bucket_rows, k)
    return lists_key_lists(data.bucket_rows) if data.name == "lists" else one_key_lists()
