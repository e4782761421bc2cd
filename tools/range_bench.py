#!/usr/bin/env python3
"""Radius queries, measured on the SIFT1M-shaped workload bench.py uses (synth.sift_manifold 10^6 x 128, the learned
16-bit hash of checkpoints/, 10^4 queries, 10 probes), one float32 index, ONE query key table for every variant.  GPU only; reads nothing
outside the repository.

Radii are chosen from the data -- the batch's own k = 256 lists -- so that a query returns about 0, 10 and 100 rows, and +inf
(everything).  Per radius, interleaved round by round with the two top-k baselines (order reversed every other round, after an untimed
warm-up round), median (min..max) over the rounds:

  count launch      bscanr_kernel in count mode alone (HIP events around the launch, recorded by nlsh_range_count)
  count call        the whole nlsh_range_count on the device: PLAN phase + candidate counts + count launch (events around the call)
  fill launch       bscanr_kernel in fill mode alone (events recorded by nlsh_range_fill)
  sort + unpack     the rest of nlsh_range_fill on the device: cursor reset, segmented sort, unpack (events around the call, minus the launch)
  range_tensors     the whole facade call, hash included, on the host clock ending in a synchronise (it reads the counts in between)
  top-k k=10/256    the baselines: the tiled scan kernel alone (`events=`), the device step of scan_tensors (PLAN + SCAN + MERGE between
                    events, check=False) and query_tensors on the host clock.  tools/isa_lint.py --compare shows these kernels to be the
                    parent commit's code line for line (profiles/range_query.txt).

    python tools/range_bench.py [--rows N] [--queries Q] [--rounds 7] [--iters 10] [--steps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nlsh_amd import _capi, io, synth  # noqa: E402
from nlsh_amd.data import SIFT  # noqa: E402
from nlsh_amd.indexer import Indexer  # noqa: E402

P = 10


def build(n_rows, Q, dev):
    corpus_h, queries_h = synth.sift_manifold(n_rows, 128, seed=synth.SEED_DATA), synth.sift_manifold(Q, 128, seed=synth.SEED_QUERY)
    Ws, bs = io.load_hasher_weights(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "checkpoints", "sift1m_manifold_h16.npz"))
    Ws, bs = [np.asarray(W, np.float32) for W in Ws], [np.asarray(b, np.float32) for b in bs]
    _, mean, std = synth.standardise(corpus_h)       # raw rows are indexed; the hash's standardisation moves into its first layer
    Ws[0] = (Ws[0] / std[None, :]).astype(np.float32)
    bs[0] = (bs[0] - Ws[0] @ mean).astype(np.float32)
    corpus, q = torch.from_numpy(corpus_h).to(dev), torch.from_numpy(queries_h).to(dev)
    ix = Indexer(io.hashing_from_weights(Ws, bs, compat=True), corpus, SIFT.distance, compat=True, algo="tiled")
    keys, nkeys = ix.hash_device(q, hash_times=P, seed=7)
    return ix, q, keys, nkeys


def spread(xs):
    xs = sorted(xs)
    return {"median": float(np.median(xs)), "min": float(xs[0]), "max": float(xs[-1])}


def fmt(s, digits=4):
    return f"{s['median']:.{digits}f} ({s['min']:.{digits}f}..{s['max']:.{digits}f})"


def events(n):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in evs:            # the library re-records the handles of events that have been recorded once
        a.record(); b.record()
    return evs


def host_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def topk_ms(ix, q, keys, nkeys, k, iters):
    """(scan kernel, device step) of scan_tensors at k, ms per launch."""
    inner, outer = events(iters), events(iters)
    for ev, (a, b) in zip(inner, outer):
        a.record()
        ix.scan_tensors(q, keys, nkeys, k=k, check=False, events=ev)
        b.record()
    torch.cuda.synchronize()
    assert int(ix.last_status.cpu()[1]) == 0, "task table overflow inside a timed region"
    return float(np.mean([a.elapsed_time(b) for a, b in inner])), float(np.mean([a.elapsed_time(b) for a, b in outer]))


class RawRange:
    """The two C calls on buffers allocated once per radius (what the facade does per call, without its host read)."""

    def __init__(self, ix, q, keys, nkeys, rad, max_tasks, window):
        L, dev, Q = _capi.lib(), q.device, q.shape[0]
        self.L, self.stream, self.Q = L, torch.cuda.current_stream(dev).cuda_stream, Q
        self.keep = (q, keys, nkeys, rad)
        self.head = ix._range_head(q, keys, nkeys, window, None, rad)
        self.ws = torch.zeros((L.nlsh_range_workspace(Q, keys.shape[1], max_tasks, ix.n_buckets, q.shape[1]),), dtype=torch.uint8, device=dev)
        self.count = torch.empty((Q,), dtype=torch.int32, device=dev)
        self.ncand = torch.empty((Q,), dtype=torch.int32, device=dev)
        self.cursor = torch.empty((Q,), dtype=torch.int32, device=dev)
        self.status = torch.zeros((2,), dtype=torch.int32, device=dev)
        self.tail = (self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(), max_tasks)
        self.run_count()
        torch.cuda.synchronize()
        assert self.status.cpu().tolist()[1] == 0
        counts = self.count.cpu().long()
        self.T = int(counts.sum())
        off = torch.zeros((Q + 1,), dtype=torch.int64)
        off[1:] = torch.cumsum(counts, 0)
        self.offsets = off.to(dev)
        self.idx = torch.empty((self.T,), dtype=torch.int32, device=dev)
        self.dist = torch.empty((self.T,), dtype=torch.float32, device=dev)
        self.sort_bytes = L.nlsh_range_sort_workspace(Q, self.T)
        self.sort_ws = torch.empty((self.sort_bytes,), dtype=torch.uint8, device=dev)

    def run_count(self, ev=(None, None)):
        _capi.check(self.L.nlsh_range_count(*self.head, self.count.data_ptr(), self.ncand.data_ptr(), *self.tail,
                                            ev[0] and ev[0].cuda_event, ev[1] and ev[1].cuda_event, self.stream))

    def run_fill(self, ev=(None, None)):
        _capi.check(self.L.nlsh_range_fill(*self.head, self.offsets.data_ptr(), self.T, self.cursor.data_ptr(), None, self.dist.data_ptr(),
                                           self.idx.data_ptr(), *self.tail, self.sort_ws.data_ptr(), self.sort_bytes,
                                           ev[0] and ev[0].cuda_event, ev[1] and ev[1].cuda_event, self.stream))

    def measure(self, iters):
        """-> ms per launch: count launch, count call, fill launch, sort + unpack (fill call minus its launch)."""
        ci, co, fi, fo = events(iters), events(iters), events(iters), events(iters)
        for j in range(iters):
            co[j][0].record()
            self.run_count(ci[j])
            co[j][1].record()
            fo[j][0].record()
            self.run_fill(fi[j])
            fo[j][1].record()
        torch.cuda.synchronize()
        assert self.status.cpu().tolist()[1] == 0
        mean = lambda evs: float(np.mean([a.elapsed_time(b) for a, b in evs]))      # noqa: E731
        fill_launch = mean(fi) if self.T else 0.0       # nothing in range: the fill call launches nothing
        return mean(ci), mean(co), fill_launch, mean(fo) - fill_launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="launches per variant and round")
    ap.add_argument("--steps", type=int, default=5, help="calls per host-clock figure and round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("range_bench needs a GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda", 0)
    ix, q, keys, nkeys = build(args.rows, args.queries, dev)
    N, Q = args.rows, args.queries
    wd, wi, wn, wk = ix.scan_tensors(q, keys, nkeys, k=256, want_keys=True)        # sizes the task table; the radii come from these lists
    max_tasks, window = ix._last_max_tasks, ix.last_window
    wd_h, wk_h = wd.cpu().numpy(), wk.cpu().numpy()
    has = lambda j: wk_h[:, j] != -1      # noqa: E731
    radii = {
        "~0 rows": float(np.quantile(wd_h[has(0), 0], 0.01)),       # the nearest candidate of 1 % of the queries
        "~10 rows": float(np.median(wd_h[has(9), 9])),              # the median 10th distance
        "~100 rows": float(np.median(wd_h[has(99), 99])),           # the median 100th distance
        "everything": float("inf"),
    }
    # held to the top-k path before anything is timed: a query's result is the dist <= r prefix of its k = 256 list (<= 256 candidates)
    light = np.flatnonzero(wn.cpu().numpy() <= 256)
    off, idx, dist, nc, _ = ix.range_scan_tensors(q, keys, nkeys, radii["~10 rows"])
    assert torch.equal(nc, wn)
    oh, ih, wi_h = off.cpu().numpy(), idx.cpu().numpy(), wi.cpu().numpy()
    for qi in light[:200].tolist():
        keep = (wk_h[qi] != -1) & (wd_h[qi] <= np.float32(radii["~10 rows"]))
        assert np.array_equal(ih[oh[qi]:oh[qi + 1]], wi_h[qi][keep]), qi
    res = {"N": N, "Q": Q, "hash_times": P, "rounds": args.rounds, "iters": args.iters, "n_buckets": ix.n_buckets,
           "candidates": int(wn.long().sum().item()), "max_tasks": int(max_tasks), "radii": {}, "topk": {}}
    raws = {}
    for name, r in radii.items():
        raws[name] = RawRange(ix, q, keys, nkeys, torch.full((Q,), r, dtype=torch.float32, device=dev), max_tasks, window)
    variants = [("k=10", 10), ("k=256", 256)] + [(name, None) for name in radii]
    run = lambda name, k: topk_ms(ix, q, keys, nkeys, k, args.iters) if k else raws[name].measure(args.iters)      # noqa: E731
    for name, k in variants:        # warm-up round
        run(name, k)
    rounds = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, k in (variants if r % 2 == 0 else variants[::-1]):
            rounds[name].append(run(name, k))
    # the whole calls on the host clock, after the device figures
    host = {name: [] for name, _ in variants}
    calls = {"k=10": lambda: ix.query_tensors(q, k=10, hash_times=P, seed=7), "k=256": lambda: ix.query_tensors(q, k=256, hash_times=P, seed=7)}
    for name, r in radii.items():
        calls[name] = (lambda r_: (lambda: ix.range_tensors(q, r_, hash_times=P, seed=7)))(r)
    for fn in calls.values():
        fn()
    for r in range(args.rounds):
        for name, _ in (variants if r % 2 == 0 else variants[::-1]):
            host[name].append(host_ms(calls[name], args.steps))
    lines = [f"sift1m: N={N} d=128 Q={Q} hash_times={P}, {ix.n_buckets} buckets, {res['candidates']} candidates per batch, task table {max_tasks}; "
             f"{args.rounds} interleaved rounds (order reversed every other round) x {args.iters} launches between HIP events, after a warm-up "
             f"round; whole calls: host clock around {args.steps} calls ending in a synchronise; ms, median (min..max)"]
    lines.append(f"  {'top-k baseline':12} {'scan kernel':>26} {'device step (plan+scan+merge)':>32} {'query_tensors (host clock)':>30}")
    for name in ("k=10", "k=256"):
        t = res["topk"][name] = {"scan_ms": spread([x[0] for x in rounds[name]]), "step_ms": spread([x[1] for x in rounds[name]]),
                                 "call_ms": spread(host[name])}
        lines.append(f"  {name:12} {fmt(t['scan_ms']):>26} {fmt(t['step_ms']):>32} {fmt(t['call_ms']):>30}")
    lines.append(f"  {'radius':12} {'rows/query':>10} {'count launch':>26} {'count call (plan+count)':>26} {'fill launch':>26} {'sort + unpack':>26} "
                 f"{'range_tensors (host clock)':>28}")
    for name, r in radii.items():
        t = res["radii"][name] = {"radius": r, "total": raws[name].T, "rows_per_query": raws[name].T / Q,
                                  "count_launch_ms": spread([x[0] for x in rounds[name]]), "count_call_ms": spread([x[1] for x in rounds[name]]),
                                  "fill_launch_ms": spread([x[2] for x in rounds[name]]), "sort_unpack_ms": spread([x[3] for x in rounds[name]]),
                                  "call_ms": spread(host[name])}
        lines.append(f"  {name:12} {t['rows_per_query']:10.2f} {fmt(t['count_launch_ms']):>26} {fmt(t['count_call_ms']):>26} {fmt(t['fill_launch_ms']):>26} "
                     f"{fmt(t['sort_unpack_ms']):>26} {fmt(t['call_ms'], 3):>28}")
    print(json.dumps(res), flush=True)
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
