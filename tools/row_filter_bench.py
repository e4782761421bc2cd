#!/usr/bin/env python3
"""Filtered queries, measured on the SIFT1M-shaped workload bench.py uses (synth.sift_manifold 10^6 x 128, the learned
16-bit hash of checkpoints/, 10^4 queries, k = 10, 10 probes), one float32 index, ONE query key table for every variant.  GPU only; reads
nothing outside the repository.  Three parts:

  1. the tiled scan kernel alone (HIP events around it, `events=`): unfiltered, and filtered with 100 / 50 / 10 / 1 % of the rows allowed,
     random filters and a contiguous id range.  Variants are interleaved round by round, the order reversed every other round, after an
     untimed warm-up round; median (min..max) over the rounds, each filtered time also as a ratio to the unfiltered kernel of the same run
     (which tools/isa_lint.py --compare shows to be the parent commit's code, line for line: profiles/row_filter.txt).
  2. `nlsh_row_filter_build` between HIP events for 10^3 / 10^5 ids and a dense mask over all rows, beside what the facade's sort and
     de-duplication of the id list costs (`torch.unique`, host clock around a synchronise) and the whole `Indexer.row_filter` call.
  3. the alternative a caller has without the feature, at the same selectivities: the unfiltered query with k' = min(256, ceil(k /
     selectivity)) and a (vectorised) host post-filter -- its time per call, the share of queries it leaves with fewer than k results
     although k allowed rows exist in the whole corpus, and recall@10 of both methods against the exact filtered ground truth
     (`exact_topk` over the allowed rows, ids mapped back).

    python tools/row_filter_bench.py [--rows N] [--queries Q] [--rounds 7] [--iters 10] [--steps 10] [--out FILE]
"""
import argparse
import json
import math
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
from nlsh_amd.exact import exact_topk  # noqa: E402
from nlsh_amd.indexer import Indexer  # noqa: E402

K, P = 10, 10
FRACTIONS = (1.0, 0.5, 0.1, 0.01)


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
    return ix, corpus, q, keys, nkeys


def spread(xs):
    xs = sorted(xs)
    return {"median": float(np.median(xs)), "min": float(xs[0]), "max": float(xs[-1])}


def fmt(s, digits=4):
    return f"{s['median']:.{digits}f} ({s['min']:.{digits}f}..{s['max']:.{digits}f})"


def scan_ms(ix, q, keys, nkeys, F, iters):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:            # (`events=` takes events that have been recorded once: the library re-records their handles)
        a.record(); b.record()
    for ev in evs:
        ix.scan_tensors(q, keys, nkeys, k=K, check=False, events=ev, filter=F)
    torch.cuda.synchronize()
    assert int(ix.last_status.cpu()[1]) == 0, "task table overflow inside a timed region"
    return float(np.mean([a.elapsed_time(b) for a, b in evs]))


def host_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def post_filter(idx_h, keys_h, allowed_h, k):
    """Unfiltered [Q, k'] lists -> the first k allowed ids of every row (-1 padded), and how many each row kept.  Vectorised numpy."""
    keep = (keys_h != -1) & allowed_h[np.clip(idx_h, 0, None)]
    rank = np.cumsum(keep, axis=1)
    take = keep & (rank <= k)
    out = np.full((idx_h.shape[0], k), -1, np.int32)
    rows, cols = np.nonzero(take)
    out[rows, rank[rows, cols] - 1] = idx_h[rows, cols]
    return out, np.minimum(rank[:, -1], k)


def recall(found, truth):
    hit = 0
    for f, t in zip(found, truth):
        hit += len(set(f[f >= 0].tolist()) & set(t[t >= 0].tolist()))
    return hit / max(int((truth >= 0).sum()), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="scan launches per variant and round")
    ap.add_argument("--steps", type=int, default=10, help="calls per host-clock figure and round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("row_filter_bench needs a GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda", 0)
    ix, corpus, q, keys, nkeys = build(args.rows, args.queries, dev)
    N, Q = args.rows, args.queries
    gen = torch.Generator(device="cpu").manual_seed(11)
    masks = {}                                  # variant -> bool [N] by id (= local row: id_base 0, no row_ids)
    for f in FRACTIONS:
        masks[f"random {100 * f:g} %"] = (torch.rand(N, generator=gen) < f) if f < 1 else torch.ones(N, dtype=torch.bool)
    for f in FRACTIONS[1:]:
        m = torch.zeros(N, dtype=torch.bool)
        m[:int(N * f)] = True
        masks[f"id range {100 * f:g} %"] = m
    filters = {name: ix.row_filter(mask=m.to(dev)) for name, m in masks.items()}
    ref = ix.scan_tensors(q, keys, nkeys, k=K, want_keys=True)          # sizes the task table; the all-allowed filter is held to its bits
    alla = ix.scan_tensors(q, keys, nkeys, k=K, want_keys=True, filter=filters["random 100 %"])
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(alla, ref)), "the all-allowed filter must give the unfiltered call's words"
    lines, res = [], {"N": N, "Q": Q, "k": K, "hash_times": P, "rounds": args.rounds, "n_buckets": ix.n_buckets,
                      "candidates": int(ref[2].long().sum().item())}

    # ---- 1. the scan kernel
    variants = [("unfiltered", None)] + list(filters.items())
    for _, F in variants:
        scan_ms(ix, q, keys, nkeys, F, 3)
    rounds = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, F in (variants if r % 2 == 0 else variants[::-1]):
            rounds[name].append(scan_ms(ix, q, keys, nkeys, F, args.iters))
    base = spread(rounds["unfiltered"])
    res["scan_ms"] = {name: dict(spread(v), ratio=float(np.median(v)) / base["median"],
                                 allowed=None if name == "unfiltered" else filters[name].n_allowed) for name, v in rounds.items()}
    lines.append(f"sift1m: N={N} d=128 Q={Q} k={K} hash_times={P}, {ix.n_buckets} buckets, {res['candidates']} candidates per batch (before any filter); "
                 f"{args.rounds} interleaved rounds (order reversed every other round) x {args.iters} scan launches between HIP events, after a warm-up round")
    lines.append(f"  {'variant':18} {'rows allowed':>12} {'scan ms median (min..max)':>30} {'x unfiltered':>13}")
    for name, r in res["scan_ms"].items():
        lines.append(f"  {name:18} {'' if r['allowed'] is None else r['allowed']:>12} {fmt(r):>30} {r['ratio']:13.3f}")

    # ---- 2. building a filter
    L, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
    words = torch.empty((L.nlsh_row_filter_words(N),), dtype=torch.int32, device=dev)
    n_allowed = torch.empty((1,), dtype=torch.int32, device=dev)
    res["build"] = {}
    lines.append(f"filter build, N={N}: nlsh_row_filter_build between HIP events; the facade's torch.unique of the id list and the whole "
                 f"Indexer.row_filter call on the host clock (ending in the call's own synchronise); median (min..max) of {args.rounds} x {args.steps}")
    for label, n_ids in (("10^3 ids", 1000), ("10^5 ids", 100_000), ("dense mask", 0)):
        if n_ids:
            raw = torch.randint(0, N, (n_ids,), generator=gen).to(dev)
            ids = torch.unique(raw).to(torch.int32)
            src = (ids.data_ptr(), int(ids.numel()), None, 0, 0)
            facade, prep = (lambda: ix.row_filter(allow=raw)), (lambda: torch.unique(raw.long()).to(torch.int32))
        else:
            m = masks["random 50 %"].to(dev)
            m8 = m.view(torch.uint8)
            src = (None, 0, m8.data_ptr(), N, 0)
            facade, prep = (lambda: ix.row_filter(mask=m)), None
        kern, prep_ms, call_ms = [], [], []
        for _ in range(args.rounds + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                _capi.check(L.nlsh_row_filter_build(ix.gid.data_ptr(), N, *src, 0, words.data_ptr(), n_allowed.data_ptr(), stream))
            b.record()
            torch.cuda.synchronize()
            kern.append(a.elapsed_time(b) / args.steps)
            if prep is not None:
                prep_ms.append(host_ms(prep, args.steps))
            call_ms.append(host_ms(facade, args.steps))
        r = res["build"][label] = {"kernel_ms": spread(kern[1:]), "unique_ms": spread(prep_ms[1:]) if prep_ms else None, "row_filter_ms": spread(call_ms[1:])}
        lines.append(f"  {label:11} kernel {fmt(r['kernel_ms'])} ms   torch.unique {fmt(r['unique_ms']) if r['unique_ms'] else '-':>26} ms   row_filter() {fmt(r['row_filter_ms'])} ms")

    # ---- 3. the alternative: over-fetch and post-filter on the host
    lines.append("filtered call against over-fetch + host post-filter (unfiltered query_tensors with k' = min(256, ceil(k / selectivity)), ids and keys "
                 "copied to the host, vectorised numpy filter); ms per call on the host clock ending in a synchronise, median (min..max); "
                 "'short': queries left with fewer than k results; recall@10 against exact_topk over the allowed rows")
    lines.append(f"  {'variant':18} {'k_over':>6} {'filtered ms/call':>28} {'short':>7} {'recall':>7}   {'over-fetch ms/call':>28} {'short':>7} {'recall':>7}")
    res["alternative"] = {}
    for name, F in filters.items():
        sel = F.n_allowed / N
        k_over = min(256, math.ceil(K / sel))
        allowed_d = masks[name].to(dev)
        allowed_h = masks[name].numpy()
        local = torch.nonzero(allowed_d).reshape(-1)
        _, ti = exact_topk(q, corpus[local], K, metric="l2")
        truth = torch.where(ti >= 0, local[ti.clamp(min=0).long()].to(torch.int32), ti).cpu().numpy()
        del local
        filt = lambda: ix.query_tensors(q, k=K, hash_times=P, seed=7, want_keys=True, filter=F)            # noqa: E731
        state = {}

        def over():
            _, i_, _, k_ = ix.query_tensors(q, k=k_over, hash_times=P, seed=7, want_keys=True)
            state["out"] = post_filter(i_.cpu().numpy(), k_.cpu().numpy(), allowed_h, K)

        filt(); over()
        tf, to = [], []
        for r in range(args.rounds):
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                (tf if which == 0 else to).append(host_ms(filt if which == 0 else over, args.steps))
        _, fi, _, fk = filt()
        f_ids = torch.where(fk != -1, fi, torch.full_like(fi, -1)).cpu().numpy()
        f_len = (fk != -1).sum(1).cpu().numpy()
        o_ids, o_len = state["out"]
        r = res["alternative"][name] = {
            "selectivity": sel, "k_over": k_over, "filtered_ms": spread(tf), "overfetch_ms": spread(to),
            "filtered_short": float((f_len < K).mean()), "overfetch_short": float((o_len < K).mean()),
            "filtered_recall": recall(f_ids, truth), "overfetch_recall": recall(o_ids, truth)}
        lines.append(f"  {name:18} {k_over:6d} {fmt(r['filtered_ms']):>28} {r['filtered_short']:7.4f} {r['filtered_recall']:7.4f}   "
                     f"{fmt(r['overfetch_ms']):>28} {r['overfetch_short']:7.4f} {r['overfetch_recall']:7.4f}")
    print(json.dumps(res), flush=True)
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
