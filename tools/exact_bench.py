#!/usr/bin/env python3
"""Time nlsh_exact_topk (nlsh_amd.exact) against the stock-torch forms it stands beside, in one process on the same tensors.

    python tools/exact_bench.py [--scale 1.0] [--rounds 5] [--out FILE]

Shapes (at --scale 1):
  ground truth  10^4 queries x 10^6 rows x 128-d, k = 10, L2         exact.exact_topk  vs  data.brute_force_topk
  GloVe-shaped  10^4 queries x 1.2 10^6 rows x 100-d, k = 10, cosine  exact.exact_topk  vs  data.brute_force_topk
  self-kNN      10^6 rows x 128-d, k = 100, L2                        exact.self_knn alone on all rows; against training.self_knn on the
                                                                      first --torch-self-rows rows (what the torch form is given to hold)
Each form is warmed up once per shape, then timed --rounds times with the two forms alternating; a time is a host clock around a call that
ends in a device synchronise.  Reported: median / min / max ms, effective fp32 TF = 2 Q N d / t, its share of the 157.3 TF matrix peak
(the whole call over the peak, not a kernel's utilisation), and torch's time over the new call's.  Rows are seeded Gaussian mixtures
generated on the device.  A measurement path without a GPU fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

PEAK_TF = 157.3


def mixture(n, d, seed, n_clusters=1000, sigma=0.35):
    g = torch.Generator(device="cuda").manual_seed(seed)
    cen = torch.randn((n_clusters, d), generator=torch.Generator(device="cuda").manual_seed(12345), device="cuda")
    which = torch.randint(0, n_clusters, (n,), generator=g, device="cuda")
    return (cen[which] + sigma * torch.randn((n, d), generator=g, device="cuda")).contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def measure(forms, rounds):
    """forms: {name: callable}; one warm-up each, then `rounds` alternating rounds.  -> {name: [ms]}, {name: last result}"""
    times, last = {n: [] for n in forms}, {}
    for n, fn in forms.items():
        timed(fn)
    for _ in range(rounds):
        for n, fn in forms.items():
            ms, last[n] = timed(fn)
            times[n].append(ms)
    return times, last


def row(name, Q, N, d, ms):
    med = statistics.median(ms)
    tf = 2.0 * Q * N * d / (med * 1e-3) / 1e12
    return dict(form=name, Q=Q, N=N, d=d, ms_median=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                effective_tf=round(tf, 2), share_of_matrix_peak=round(tf / PEAK_TF, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every row and query count (rehearsals)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-self-rows", type=int, default=131072)
    ap.add_argument("--out", default=None, help="also write the result lines to this file (profiles/exact_knn.txt holds such a run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exact_bench needs a GPU: nothing is measured without one")
    from nlsh_amd import data, exact, training

    sc = lambda n: max(256, int(n * args.scale))   # noqa: E731
    results = []

    def versus(tag, q, c, k, metric):
        Q, N, d = q.shape[0], c.shape[0], c.shape[1]
        forms = {"exact.exact_topk": lambda: exact.exact_topk(q, c, k, metric=metric)[1],
                 "data.brute_force_topk": lambda: data.brute_force_topk(q, c, k, metric)}
        times, last = measure(forms, args.rounds)
        a, b = last["exact.exact_topk"].to(torch.int64), last["data.brute_force_topk"]
        same = (a.sort(1).values == b.sort(1).values).float().mean().item()   # both exact up to fp32 near-ties
        new, old = row("exact.exact_topk", Q, N, d, times["exact.exact_topk"]), row("data.brute_force_topk", Q, N, d, times["data.brute_force_topk"])
        results.append(dict(shape=tag, k=k, metric=metric, new=new, torch=old, torch_over_new=round(old["ms_median"] / new["ms_median"], 3),
                            id_agreement=round(same, 6), workspace_bytes=exact.workspace_bytes(Q, N, k)))
        print(json.dumps(results[-1]), flush=True)

    c = mixture(sc(1_000_000), 128, 1)
    q = mixture(sc(10_000), 128, 2)
    versus("ground truth", q, c, 10, "l2")

    # self-kNN on the same corpus: the new form on all rows, both forms on a leading row range
    n_sub = min(c.shape[0], sc(args.torch_self_rows))
    sub = c[:n_sub]
    times, last = measure({"exact.self_knn": lambda: exact.self_knn(c, 100)}, max(1, args.rounds // 2))
    full = row("exact.self_knn", c.shape[0], c.shape[0], 128, times["exact.self_knn"])
    times, last = measure({"exact.self_knn": lambda: exact.self_knn(sub, 100), "training.self_knn": lambda: training.self_knn(sub, 100)},
                          args.rounds)
    a, b = last["exact.self_knn"], last["training.self_knn"]
    same = (a.sort(1).values == b.sort(1).values).float().mean().item()
    new, old = row("exact.self_knn", n_sub, n_sub, 128, times["exact.self_knn"]), row("training.self_knn", n_sub, n_sub, 128, times["training.self_knn"])
    results.append(dict(shape="self-kNN", k=100, metric="l2", new_all_rows=full, new=new, torch=old,
                        torch_over_new=round(old["ms_median"] / new["ms_median"], 3), id_agreement=round(same, 6),
                        workspace_bytes_all_rows=exact.workspace_bytes(c.shape[0], c.shape[0], 100)))
    print(json.dumps(results[-1]), flush=True)
    del c, q, sub, a, b, last
    torch.cuda.empty_cache()

    c = mixture(sc(1_200_000), 100, 3, sigma=0.6)
    q = mixture(sc(10_000), 100, 4, sigma=0.6)
    versus("GloVe-shaped", q, c, 10, "cosine")

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"# tools/exact_bench.py --scale {args.scale} --rounds {args.rounds}; {torch.cuda.get_device_name(0)}; times in ms, host clock "
                    f"around a synchronised call, median (min .. max) of {args.rounds} alternating rounds after one warm-up; TF = 2 Q N d / t over "
                    f"the whole call; matrix peak {PEAK_TF} TF\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
    slower = [r["shape"] for r in results if r["torch_over_new"] < 1.0]
    print("RESULT " + json.dumps(dict(shapes=len(results), new_call_slower_than_torch_on=slower)), flush=True)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
