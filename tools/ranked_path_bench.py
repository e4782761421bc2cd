#!/usr/bin/env python
"""The ranked mode's one-call path (`nlsh_query_batch_ranked`: five launches, the keys looked up by the kernel that ranks them) against
its two-step path (`hash_device` / `nlsh_probe_ranked[_budget]` + `scan_tensors`: seven launches), A/B in ONE process
(profiles/ranked_one_call.txt).

    python tools/ranked_path_bench.py [--repeats 60] [--rows ranked10,ranked32,budget3000]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ranked_path_bench.py --trace-only --rows ranked10 --repeats 20

Workload: the SIFT1M-shaped one of tools/eval_curve.py (10^6 x 128-d `synth.sift_manifold` rows, 10^4 queries, the 16-bit hash of
checkpoints/sift1m_manifold_h16.npz, k = 10, compat=False).  Rows: ranked at hash_times 10 and 32, candidate_budget 3000 at cap 64.
Per row, after a warm-up of both paths, the two paths ALTERNATE by the class switch `Indexer.ranked_one_call`, `--repeats` times each:
  (a) device_ms   `query_tensors(check=False)` between two device events (the batch's launches on the stream, results device-resident);
  (b) query_ms    `query()` on the host clock; the call ends in its own stream synchronisation and returns the Python lists.
One JSON line per row: median, 10th / 90th percentile, min and max of each quantity and path, the medians of the even and the odd repeats
of the same path (what two runs of the SAME code differ by), and whether the two paths returned identical results at this size (the
whole id / distance-bit / count tensors of `query_tensors`, the first and the last id list and all counts of `query()`).
--trace-only: no timing, `--repeats` `query_tensors(check=False)` calls per path and row, for a kernel trace of the run.
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

ROWS = {"ranked10": (10, None), "ranked32": (32, None), "budget3000": (64, 3000)}


def stats(v):
    a = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)), "min": float(a.min()),
            "max": float(a.max()), "median_even": float(np.median(a[0::2])), "median_odd": float(np.median(a[1::2])), "n": int(len(a))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="checkpoints/sift1m_manifold_h16.npz")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--q", type=int, default=10_000)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ranked_path_bench needs the GPU: nothing here can be timed without one")
    from nlsh_amd import io as nio, synth
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer

    model = args.model if os.path.exists(args.model) else os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", args.model)
    Ws, bs = nio.load_hasher_weights(model)
    corpus, mean, std = synth.standardise(synth.sift_manifold(args.n, 128))
    queries, _, _ = synth.standardise(synth.sift_manifold(args.q, 128, seed=synth.SEED_QUERY), mean, std)
    cg, qg = torch.from_numpy(corpus).cuda(), torch.from_numpy(queries).cuda()
    ix = Indexer(nio.hashing_from_weights(Ws, bs, compat=False), cg, SIFT.distance, compat=False)
    torch.cuda.synchronize()
    print(f"# index: {ix.bucket_stats()}, {args.q} queries, k={args.k}, repeats={args.repeats}", flush=True)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def tensors(one_call, P, budget):
        Indexer.ranked_one_call = one_call
        ev0.record()
        out = ix.query_tensors(qg, k=args.k, hash_times=P, probes="ranked", candidate_budget=budget, check=False)
        ev1.record()
        ev1.synchronize()
        assert ix.last_query_path == ("ranked_one_call" if one_call else "two_step"), ix.last_query_path
        return ev0.elapsed_time(ev1), out

    def lists(one_call, P, budget):
        Indexer.ranked_one_call = one_call
        t0 = time.perf_counter()
        out = ix.query(qg, k=args.k, hash_times=P, probes="ranked", candidate_budget=budget)
        dt = (time.perf_counter() - t0) * 1e3
        assert ix.last_query_path == ("ranked_one_call" if one_call else "two_step"), ix.last_query_path
        return dt, out

    for name in [r for r in args.rows.split(",") if r]:
        P, budget = ROWS[name]
        # task tables sized, code objects loaded, kept plans built: both paths, checked calls first
        for one_call in (True, False):
            Indexer.ranked_one_call = one_call
            ix.query_tensors(qg, k=args.k, hash_times=P, probes="ranked", candidate_budget=budget)
            for _ in range(args.warmup):
                tensors(one_call, P, budget)
                if not args.trace_only:
                    lists(one_call, P, budget)
        if args.trace_only:
            for _ in range(args.repeats):
                for one_call in (True, False):
                    tensors(one_call, P, budget)
            print(json.dumps({"row": name, "hash_times": P, "candidate_budget": budget, "trace_only": True, "calls_per_path": args.repeats + args.warmup + 1}), flush=True)
            continue
        # results: the two paths at this size
        (_, a), (_, b) = tensors(True, P, budget), tensors(False, P, budget)
        same_tensors = bool(torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[2], b[2]))
        mean_cand = float(a[2].float().mean())
        (_, la), (_, lb) = lists(True, P, budget), lists(False, P, budget)
        same_lists = bool(la[0][0] == lb[0][0] and la[0][-1] == lb[0][-1] and la[1] == lb[1])
        del a, b, la, lb
        dev = {True: [], False: []}
        host = {True: [], False: []}
        for _ in range(args.repeats):
            for one_call in (True, False):
                dev[one_call].append(tensors(one_call, P, budget)[0])
            for one_call in (True, False):
                host[one_call].append(lists(one_call, P, budget)[0])
        print(json.dumps({"row": name, "hash_times": P, "candidate_budget": budget, "mean_candidates": mean_cand,
                          "same_tensors": same_tensors, "same_first_last_lists_and_counts": same_lists,
                          "device_ms": {"one_call": stats(dev[True]), "two_step": stats(dev[False])},
                          "query_ms": {"one_call": stats(host[True]), "two_step": stats(host[False])}}), flush=True)
    Indexer.ranked_one_call = True


if __name__ == "__main__":
    main()
