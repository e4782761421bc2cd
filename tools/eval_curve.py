#!/usr/bin/env python3
"""The reference's offline evaluation flow (eval.py:103-197) on the HIP path: load a hasher, hash the
corpus, build the index, then for n_samples = 1..N probe keys per query report the mean number of
candidates and recall@K -- the recall-vs-candidates trade-off curve eval.py prints (eval.py:196).

    python tools/eval_curve.py --model checkpoints/sift1m_manifold_h16.npz --data synth:sift1m [--max-samples 32]
    python tools/eval_curve.py --model run_cpu.pt --base base.fvecs --query query.fvecs --gt gt.ivecs --metric l2
    python tools/eval_curve.py --model checkpoints/sift1m_manifold_h16.npz --data synth:sift1m --probes ranked
    python tools/eval_curve.py --model checkpoints/sift1m_manifold_h16.npz --data synth:sift1m --candidate-budget 500,1000,2000,4000

--probes ranked probes the n_samples most probable codes in descending probability (nlsh_probe_ranked) instead of the Philox draws:
n_samples distinct buckets per query and no seed.  avg_n_keys is the mean number of distinct keys a query probes.
--candidate-budget B[,B...] (implies --probes ranked) adds one row per budget behind the fixed-n rows: every query probes its ranked keys
until their buckets hold B candidates (`Indexer.query_tensors(candidate_budget=B)`, at most --budget-cap keys).  Every row, fixed-n or
budgeted, carries the same columns -- mean, median and maximum of keys and of candidates per query, recall, and the share of queries
with fewer than K candidates -- so the two can be read at equal mean candidates without interpolation.

Differences from eval.py, on purpose: keys are full width (eval.py's `_binarr_to_int`, eval.py:49-53),
every query is multi-probed (no trailing-batch rule), `<K` candidates return all of them (eval.py:185-186).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True, help=".npz | TorchScript _cpu.pt | state dict")
    ap.add_argument("--data", default=None, help="synth:sift1m | synth:glove (seeded generators of bench.py)")
    ap.add_argument("--base"); ap.add_argument("--query"); ap.add_argument("--gt")
    ap.add_argument("--metric", default=None, choices=["l2", "cosine"])
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--max-samples", type=int, default=32)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--q", type=int, default=10000)
    ap.add_argument("--tanh", action="store_true")
    ap.add_argument("--seed", type=int, default=1, help="Philox seed of the probes: one stream, so the probe sets are nested in n_samples")
    ap.add_argument("--probes", default="sampled", choices=["sampled", "ranked"],
                    help="sampled: Bernoulli draws (the reference's form) | ranked: the n_samples most probable codes (no seed)")
    ap.add_argument("--candidate-budget", default="", help="B[,B...]: candidate budgets of ranked probes (implies --probes ranked)")
    ap.add_argument("--budget-cap", type=int, default=128, help="hash_times of the budgeted rows: the most keys a query may probe")
    args = ap.parse_args()
    budgets = [int(v) for v in args.candidate_budget.split(",") if v]
    if budgets:
        args.probes = "ranked"
    from nlsh_amd import io as nio, synth
    from nlsh_amd.data import Glove, SIFT, brute_force_topk
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.metrics import calculate_recall

    model = args.model if os.path.exists(args.model) else os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", args.model)
    Ws, bs = nio.load_hasher_weights(model)
    if args.data == "synth:sift1m":
        n = args.n or 1_000_000
        corpus, mean, std = synth.standardise(synth.sift_manifold(n, 128))
        queries, _, _ = synth.standardise(synth.sift_manifold(args.q, 128, seed=synth.SEED_QUERY), mean, std)
        metric = "l2"
    elif args.data == "synth:glove":
        corpus, queries, metric = synth.glove_manifold(args.n or 1_183_514, 100), synth.glove_manifold(args.q, 100, seed=synth.SEED_QUERY), "cosine"
    else:
        rd = lambda p: nio.read_bvecs(p) if p.endswith(".bvecs") else nio.read_fvecs(p)  # noqa: E731
        corpus, queries, metric = rd(args.base), rd(args.query), args.metric or "l2"
    metric = args.metric or metric
    cg, qg = torch.from_numpy(corpus).cuda(), torch.from_numpy(queries).cuda()
    gt = nio.read_ivecs(args.gt)[:, :args.k] if args.gt else brute_force_topk(qg, cg, args.k, metric).cpu().numpy()

    hashing = nio.hashing_from_weights(Ws, bs, tanh_output=args.tanh, compat=False)
    t0 = time.time()
    indexer = Indexer(hashing, cg, SIFT.distance if metric == "l2" else Glove.distance, compat=False)
    torch.cuda.synchronize()
    print(f"# index: {indexer.bucket_stats()} built in {time.time() - t0:.3f}s", flush=True)
    print("n_samples avg_n_candidates recall qps avg_n_keys med_n_keys max_n_keys med_n_candidates max_n_candidates share_below_k")
    rows = []

    def measure(label, hash_times, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dist, idx, nc, _ = indexer.query_tensors(qg, k=args.k, hash_times=hash_times, seed=args.seed, probes=args.probes, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        _, nkeys = indexer.hash_device(qg, hash_times=hash_times, seed=args.seed, probes=args.probes, **kw)    # the same keys again, for their count
        ids = [r[r >= 0].tolist() for r in idx.cpu().numpy()]
        rec = float(np.mean(calculate_recall(list(gt), ids)))
        nk, ncf = nkeys.float(), nc.float()
        row = {"avg_n_candidates": float(ncf.mean()), "recall": rec, "qps": len(ids) / dt, "avg_n_keys": float(nk.mean()),
               "med_n_keys": float(nk.median()), "max_n_keys": int(nkeys.max()), "med_n_candidates": float(ncf.median()),
               "max_n_candidates": int(nc.max()), "share_below_k": float((nc < args.k).float().mean())}
        print(label, f"{row['avg_n_candidates']:.1f}", f"{rec:.4f}", f"{row['qps']:.0f}", f"{row['avg_n_keys']:.3f}", f"{row['med_n_keys']:.0f}",
              row["max_n_keys"], f"{row['med_n_candidates']:.0f}", row["max_n_candidates"], f"{row['share_below_k']:.4f}", flush=True)
        return row

    for n_samples in range(1, min(args.max_samples, 100) + 1):   # eval.py:148 range(1, 101)
        rows.append({"n_samples": n_samples, **measure(n_samples, n_samples)})
    budget_rows = []
    if budgets:
        print(f"# candidate budgets, at most {args.budget_cap} keys per query; the columns are those of the fixed-n rows above")
    for b in budgets:
        budget_rows.append({"candidate_budget": b, "cap": args.budget_cap, **measure(f"budget={b}", args.budget_cap, candidate_budget=b)})
    print(json.dumps({"model": args.model, "metric": metric, "k": args.k, "probes": args.probes, "curve": rows, **({"budget_curve": budget_rows} if budgets else {})}))


if __name__ == "__main__":
    main()
