#!/usr/bin/env python3
"""Multi-table indexes measured on the GPU (writes the text of profiles/multi_table.txt):

(a) `nlsh_merge_topk_unique` against `nlsh_merge_topk` on the same DISJOINT input (both produce the same output there) at Q = 10^4,
    k in {10, 100}, G in {2, 4, 8, 16}, plus a fully overlapping input (all G lists identical) for the unique kernel alone: device
    events around bursts of launches, the two kernels alternating in one process, median and minimum over the rounds -- beside one
    table's whole device step (`Indexer.query_tensors`, hash + scan + merge) at the same Q and k.
(b) recall@10 against mean SCORED candidates per query on the SIFT1M-shaped synthetic workload for T in {1, 2, 4} tables x
    hash_times in {1, 2, 5, 10}, sampled and ranked probes, each T > 1 row beside the single-table ranked row of nearest candidate
    count, with the wall time per batch and the peak device memory of the configuration.  The T hashes are trained here with
    tools/train_hash.py's recipe (`training.fit_triplet`, 16 bits, 256-256 MLP) and differ in their seed alone; T = 1 uses the first.

    python tools/multi_table_bench.py --out profiles/multi_table.txt [--steps 1500] [--n 1000000] [--q 10000] [--part all|merge|recall]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def median_min(v):
    return float(np.median(v)), float(np.min(v))


def event_ms(fn, bursts=15, per_burst=20, warmup=3):
    """ms per call of `fn`: device events around bursts of back-to-back calls -> one figure per burst."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(bursts):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per_burst):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / per_burst)
    return out


def merge_inputs(G, Q, k, overlap):
    """int64 [G, Q, k] ascending lists of real keys: disjoint (every key its own id) or all G lists identical."""
    gen = torch.Generator(device="cuda").manual_seed(G * 1000 + k)
    n = 1 if overlap else G
    dist = torch.randint(1 << 20, 1 << 30, (n, Q, k), generator=gen, device="cuda", dtype=torch.int64)
    ids = torch.arange(n * k, device="cuda", dtype=torch.int64).view(n, 1, k).expand(n, Q, k)
    keys = torch.sort((dist << 32) | ids, dim=2).values
    return (keys.expand(G, Q, k) if overlap else keys).contiguous()


def part_merge(args, step_ms):
    from nlsh_amd import _capi
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    Q = args.q
    say("(a) merge kernel time, Q = %d queries, ms per launch: median (min) over 15 bursts of 20 launches, the kernels alternating" % Q)
    say("    unique = nlsh_merge_topk_unique, plain = nlsh_merge_topk (the parent's merge of disjoint lists); same input, same output words")
    say("  k    G   plain disjoint     unique disjoint    unique/plain   unique, all lists identical   one table's device step (ranked, 10 probes)")
    for k in (10, 100):
        for G in (2, 4, 8, 16):
            od = torch.empty((Q, k), dtype=torch.float32, device="cuda")
            oi = torch.empty((Q, k), dtype=torch.int32, device="cuda")
            od2, oi2 = torch.empty_like(od), torch.empty_like(oi)
            dis, same = merge_inputs(G, Q, k, False), merge_inputs(G, Q, k, True)

            def plain(x=dis):
                _capi.check(L.nlsh_merge_topk(x.data_ptr(), k, G, Q, k, None, od.data_ptr(), oi.data_ptr(), None, stream))

            def unique(x=dis, d=od2, i=oi2):
                _capi.check(L.nlsh_merge_topk_unique(x.data_ptr(), k, G, Q, k, None, d.data_ptr(), i.data_ptr(), None, None, stream))

            plain(); unique()
            torch.cuda.synchronize()
            assert torch.equal(od.view(torch.int32), od2.view(torch.int32)) and torch.equal(oi, oi2), "the two merges differ on disjoint input"
            tp, tu = [], []
            for _ in range(3):                      # interleaved rounds
                tp += event_ms(plain, bursts=5)
                tu += event_ms(unique, bursts=5)
            to = event_ms(lambda: unique(same))
            (pm, pn), (um, un), (om, on) = median_min(tp), median_min(tu), median_min(to)
            step = step_ms.get(k)
            say("%3d  %3d   %.4f (%.4f)    %.4f (%.4f)    %5.2f          %.4f (%.4f)               %s"
                % (k, G, pm, pn, um, un, um / pm, om, on, "not measured" if step is None else "%.3f (%.3f)" % step))
    say()


def train_hashes(args, cg, T):
    from nlsh_amd import exact, training
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.hashings import MultivariateBernoulli
    t0 = time.time()
    knn = exact.self_knn(cg, 10, metric="l2")
    torch.cuda.synchronize()
    say("    self-kNN (k = 10, nlsh_exact_topk) of the %d training rows: %.1f s" % (cg.shape[0], time.time() - t0))
    out = []
    for t in range(T):
        torch.manual_seed(t)
        h = MultivariateBernoulli(MultiLayerRelu(cg.shape[1], [256, 256]), 16, None, compat=True)
        t0 = time.time()
        training.fit_triplet(h, cg, knn, n_steps=args.steps, seed=t, log=lambda s: None)
        torch.cuda.synchronize()
        h.train_mode(False)
        say("    hash %d: seed %d, %d triplet steps in %.1f s" % (t, t, args.steps, time.time() - t0))
        out.append(h)
    return out


def part_recall(args):
    from nlsh_amd import synth
    from nlsh_amd.data import SIFT, brute_force_topk
    from nlsh_amd.metrics import calculate_recall
    from nlsh_amd.multitable import MultiTableIndexer
    corpus, mean, std = synth.standardise(synth.sift_manifold(args.n, 128))
    queries, _, _ = synth.standardise(synth.sift_manifold(args.q, 128, seed=synth.SEED_QUERY), mean, std)
    cg, qg = torch.from_numpy(corpus).cuda(), torch.from_numpy(queries).cuda()
    gt = list(brute_force_topk(qg, cg, 10, "l2").cpu().numpy())
    say("(b) recall@10 against mean scored candidates per query: synth.sift_manifold, %d x 128-d standardised rows, %d queries, L2, float32 storage" % (args.n, args.q))
    say("    hashes: 16 bits, 256-256 MLP, tools/train_hash.py's triplet recipe at %d steps each (the shipped checkpoint: 6000), seeds 0..3;" % args.steps)
    say("    T = 1 is hash 0 through the same MultiTableIndexer path.  hash_times is PER TABLE; candidates are scored pairs, with multiplicity")
    hashers = train_hashes(args, cg, 4)
    base = torch.cuda.memory_allocated()

    def measure(mt, hash_times, probes):
        kw = dict(k=10, hash_times=hash_times, probes=probes, seed=1)
        mt.query_tensors(qg, **kw)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        wall = []
        for _ in range(5):
            t0 = time.perf_counter()
            _, idx, nc, keys = mt.query_tensors(qg, want_keys=True, **kw)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        ids = [r[m].tolist() for r, m in zip(idx.cpu().numpy(), (keys != -1).cpu().numpy())]
        return dict(cand=float(nc.float().mean()), recall=float(np.mean(calculate_recall(gt, ids))), ms=float(np.median(wall)),
                    peak_gb=(torch.cuda.max_memory_allocated() - base) / 1e9)

    rows, step_ms = {}, {}
    single = []
    for T in (1, 2, 4):
        mt = MultiTableIndexer(hashers[:T], cg, SIFT.distance)
        torch.cuda.synchronize()
        say("    T = %d: %s" % (T, ", ".join("%d buckets" % t.n_buckets for t in mt.tables)))
        if T == 1:
            for P in (1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 64):     # the single-table ranked curve the rows below are held against
                single.append((P, measure(mt, P, "ranked")))
            for k in (10, 100):
                ms = event_ms(lambda: mt.tables[0].query_tensors(qg, k=k, hash_times=10, probes="ranked", check=False), bursts=9, per_burst=5)
                step_ms[k] = median_min(ms)
        for probes in ("sampled", "ranked"):
            for P in (1, 2, 5, 10):
                rows[(T, probes, P)] = measure(mt, P, probes)
        del mt
        torch.cuda.empty_cache()
    say()
    say("    single table, ranked probes (the yardstick):")
    say("    hash_times  candidates  recall@10  ms/batch")
    for P, r in single:
        say("    %10d  %10.1f  %9.4f  %8.3f" % (P, r["cand"], r["recall"], r["ms"]))
    say()
    say("    T  probes   hash_times  candidates  recall@10  ms/batch  peak GB | single-table ranked row of nearest candidates: hash_times candidates recall@10 ms/batch")
    wins = {"tables": 0, "probes": 0, "tie": 0}
    for (T, probes, P), r in rows.items():
        near = min(single, key=lambda s: abs(s[1]["cand"] - r["cand"]))
        say("    %d  %-7s  %10d  %10.1f  %9.4f  %8.3f  %7.2f | %3d %10.1f %9.4f %8.3f"
            % (T, probes, P, r["cand"], r["recall"], r["ms"], r["peak_gb"], near[0], near[1]["cand"], near[1]["recall"], near[1]["ms"]))
        if T > 1 and probes == "ranked":
            # compare at EQUAL candidates: the single-table recall interpolated at this row's candidate count
            xs, ys = [s[1]["cand"] for s in single], [s[1]["recall"] for s in single]
            if xs[0] <= r["cand"] <= xs[-1]:
                at = float(np.interp(r["cand"], xs, ys))
                wins["tables" if r["recall"] > at + 0.002 else "probes" if r["recall"] < at - 0.002 else "tie"] += 1
                say("       at %.1f candidates one table's ranked curve interpolates to recall %.4f: %+.4f for %d tables" % (r["cand"], at, r["recall"] - at, T))
    say()
    say("    ranked rows with T > 1 against one table at equal candidates (+-0.002 = tie): more tables won %d, more probes won %d, ties %d"
        % (wins["tables"], wins["probes"], wins["tie"]))
    say()
    return step_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/multi_table.txt")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--q", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--part", default="all", choices=["all", "merge", "recall"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("multi_table_bench.py measures on the GPU: no device, no numbers")
    say("# tools/multi_table_bench.py --n %d --q %d --steps %d --part %s   (%s)" % (args.n, args.q, args.steps, args.part, torch.cuda.get_device_name(0)))
    say()
    step_ms = part_recall(args) if args.part in ("all", "recall") else {}
    if args.part in ("all", "merge"):
        part_merge(args, step_ms)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
