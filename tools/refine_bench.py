#!/usr/bin/env python3
"""Exact re-ranking measured (profiles/refine.txt is made from this): three tables per workload, every configuration of a
table timed in ONE process, interleaved round by round, medians and min..max over the rounds.  GPU only; reads nothing outside the
repository.  Nothing here is a pass bar.

Workloads: tools/storage_bench.py's (same generators, same learned or seeded hashes), 10^4 queries, 10 probes, k = 10.  The float32 index
holds the ORIGINAL rows (not float16-rounded ones: the point of the stage is the caller's rows); the sq8 and the folded index share its
bucket keys and every configuration shares one query key table.

  1. the re-rank kernel alone at k1 = 20, 40, 100, 256 on the sq8 index's own stage-one lists: device store and host store (HIP events
     around `iters` launches), the bytes of the gathered rows per second, beside `torch.index_select` of the same rows from the same
     device store and beside a device copy of as many bytes;
  2. the whole `query_tensors` call: sq8 + refine | plain sq8 | plain float32, and folded + refine | plain folded | exact;
  3. recall@10 against the float32 lists at the same probes: sq8 unrefined and at refine_factor 1, 2, 4, 10, and a 4-table
     `MultiTableIndexer` (seeded hashes) unrefined and refined against its float32 twin.

    python tools/refine_bench.py [--workloads sift1m,glove,deep] [--rows N] [--rounds 5] [--iters 10] [--steps 20] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nlsh_amd import io, synth  # noqa: E402
from nlsh_amd.data import Glove, SIFT  # noqa: E402
from nlsh_amd.indexer import Indexer  # noqa: E402
from nlsh_amd.multitable import MultiTableIndexer  # noqa: E402
from nlsh_amd.refine import RefineStore  # noqa: E402
from storage_bench import WORKLOADS, recall_at_k, spread  # noqa: E402

K, P = 10, 10
K1S = (20, 40, 100, 256)
FACTORS = (1, 2, 4, 10)


def hasher_weights(w, corpus_h, seed=None):
    """The workload's learned hash (seed None) or a seeded random one, its input standardisation folded into the first layer."""
    d = corpus_h.shape[1]
    if w["ckpt"] and seed is None:
        Ws, bs = io.load_hasher_weights(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "checkpoints", w["ckpt"]))
        fold = w["metric"] == "l2"
    else:
        Ws, bs = synth.make_weights([d, 256, 16], gain=4.0, **({} if seed is None else {"seed": seed}))
        fold = True
    Ws, bs = [np.asarray(W, np.float32) for W in Ws], [np.asarray(b, np.float32) for b in bs]
    if fold:
        _, mean, std = synth.standardise(corpus_h)
        Ws[0] = (Ws[0] / std[None, :]).astype(np.float32)
        bs[0] = (bs[0] - Ws[0] @ mean).astype(np.float32)
    return Ws, bs


def event_ms(fn, iters):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return float(np.mean([a.elapsed_time(b) for a, b in evs]))


def batch_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def interleaved(configs, rounds, measure):
    """{name: fn} -> {name: spread of `measure(fn)` over the rounds}, A B C A B C ..., one untimed warm-up round first."""
    got = {name: [] for name in configs}
    for r in range(rounds + 1):
        for name, fn in configs.items():
            v = measure(fn)
            if r:
                got[name].append(v)
    return {name: spread(v) for name, v in got.items()}


def fmt(s):
    return f"{s['median']:9.4f} ({s['min']:.4f}..{s['max']:.4f})"


def run(tag, args, dev, lines):
    w = WORKLOADS[tag]
    N, d = args.rows or w["N"], w["d"]
    gen = getattr(synth, w["gen"])
    corpus_h, queries_h = gen(N, d, seed=synth.SEED_DATA), gen(args.queries, d, seed=synth.SEED_QUERY)
    dist = SIFT.distance if w["metric"] == "l2" else Glove.distance
    hashing = io.hashing_from_weights(*hasher_weights(w, corpus_h), compat=w["compat"])
    rows, q = torch.from_numpy(corpus_h).to(dev), torch.from_numpy(queries_h).to(dev)
    f32 = Indexer(hashing, rows, dist, compat=w["compat"], algo="tiled")
    sq8 = Indexer(hashing, rows, dist, compat=w["compat"], storage="sq8", corpus_keys=f32.corpus_keys, refine="device")
    keys, nkeys = f32.hash_device(q, hash_times=P, seed=7)
    lines.append(f"{tag}: N={N} d={d} Q={args.queries} k={K} hash_times={P} metric={w['metric']}, {f32.n_buckets} buckets; {args.rounds} interleaved rounds")

    # ---- 1. the kernel alone
    store_d = sq8.refine_store
    store_h = RefineStore(rows, w["metric"], where="host")
    lines.append(f"  1. re-rank kernel alone ({args.iters} launches per round; GB/s = bytes of the gathered rows, d x 4 each)")
    lines.append(f"     {'k1':>4} {'rows':>9} {'device store ms':>28} {'GB/s':>7} {'host store ms':>28} {'GB/s':>7} {'index_select ms':>28} {'GB/s':>7} {'device copy ms':>28} {'GB/s':>7}")
    for k1 in K1S:
        cand = sq8.scan_tensors(q, keys, nkeys, k=k1, refine_k=0)[1].contiguous()
        n_valid = int((cand >= 0).sum().item())
        flat = cand.reshape(-1)
        sel = flat[flat >= 0].long()
        src = torch.empty((max(n_valid, 1), store_d.stride), dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)
        a = store_d.rerank(q, cand, K, check=False)
        b = store_h.rerank(q, cand, K, check=False)
        assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))
        res = interleaved({"device": lambda: store_d.rerank(q, cand, K, check=False), "host": lambda: store_h.rerank(q, cand, K, check=False),
                           "select": lambda: torch.index_select(store_d.rows, 0, sel), "copy": lambda: dst.copy_(src)},
                          args.rounds, lambda fn: event_ms(fn, args.iters))
        gb = lambda name, passes=1: n_valid * d * 4 * passes / (res[name]["median"] * 1e-3) / 1e9   # noqa: E731
        lines.append(f"     {k1:4d} {n_valid:9d} {fmt(res['device']):>28} {gb('device'):7.0f} {fmt(res['host']):>28} {gb('host'):7.1f} "
                     f"{fmt(res['select']):>28} {gb('select'):7.0f} {fmt(res['copy']):>28} {gb('copy'):7.0f}")
        del src, dst
    del store_h

    # ---- 2. the whole call
    lines.append(f"  2. query_tensors, ms per batch ({args.steps} batches per round, host clock, one synchronise at the end)")
    call = lambda ix, **kw: (lambda i: ix.query_tensors(q, k=K, hash_times=P, seed=100 + i, check=False, **kw))   # noqa: E731
    configs = {"sq8 + refine (k1 = 40)": call(sq8), "sq8": call(sq8, refine_k=0), "float32 exact": call(f32)}
    if w["metric"] == "l2":
        folded = Indexer(hashing, rows, dist, compat=w["compat"], algo="tiled", l2_form="folded", corpus_keys=f32.corpus_keys, refine="device")
        configs.update({"folded + refine (k1 = 40)": call(folded), "folded": call(folded, refine_k=0)})
    for ix in (sq8, f32) + ((folded,) if w["metric"] == "l2" else ()):
        ix.query_tensors(q, k=K, hash_times=P, seed=7)       # checked calls size the task tables
        if ix.refine_store is not None:
            ix.query_tensors(q, k=K, hash_times=P, seed=7, refine_k=0)
    res = interleaved(configs, args.rounds, lambda fn: batch_ms(fn, args.steps))
    for name, s in res.items():
        lines.append(f"     {name:28} {fmt(s)}   x float32 {s['median'] / res['float32 exact']['median']:.3f}")
    if w["metric"] == "l2":
        del folded

    # ---- 3. recall@10 against the float32 lists at the same probes
    F = f32.scan_tensors(q, keys, nkeys, k=K)[1]
    parts = [f"unrefined {recall_at_k(sq8.scan_tensors(q, keys, nkeys, k=K, refine_k=0)[1], F):.4f}"]
    for f in FACTORS:
        parts.append(f"factor {f} {recall_at_k(sq8.scan_tensors(q, keys, nkeys, k=K, refine_k=K * f)[1], F):.4f}")
    lines.append(f"  3. recall@{K} of sq8 against the float32 lists: " + ", ".join(parts))
    del sq8, f32
    torch.cuda.empty_cache()
    hashers = [io.hashing_from_weights(*hasher_weights(w, corpus_h, seed=500 + t), compat=False) for t in range(4)]
    mt32 = MultiTableIndexer(hashers, rows, dist)
    mt8 = MultiTableIndexer(hashers, rows, dist, storage="sq8", corpus_keys=[t.corpus_keys for t in mt32.tables], refine="device")
    kw = dict(k=K, hash_times=3, probes="ranked")
    F = mt32.query_tensors(q, **kw)[1]
    parts = [f"unrefined {recall_at_k(mt8.query_tensors(q, refine_k=0, **kw)[1], F):.4f}"]
    for f in FACTORS:
        parts.append(f"factor {f} {recall_at_k(mt8.query_tensors(q, refine_k=K * f, **kw)[1], F):.4f}")
    res = interleaved({"refined": lambda i: mt8.query_tensors(q, **kw), "unrefined": lambda i: mt8.query_tensors(q, refine_k=0, **kw),
                       "float32": lambda i: mt32.query_tensors(q, **kw)}, args.rounds, lambda fn: batch_ms(fn, max(args.steps // 4, 2)))
    lines.append(f"     MultiTableIndexer, T = 4 seeded hashes, 3 ranked probes per table, sq8 against its float32 twin: " + ", ".join(parts))
    lines.append(f"     ms per batch: sq8 + refine {fmt(res['refined'])}, sq8 {fmt(res['unrefined'])}, float32 {fmt(res['float32'])}")
    del mt8, mt32
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sift1m,glove,deep")
    ap.add_argument("--rows", type=int, default=0, help="rows of every workload (default: its own size)")
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("refine_bench needs a GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda", 0)
    lines = []
    for tag in args.workloads.split(","):
        n0 = len(lines)
        run(tag, args, dev, lines)
        print("\n".join(lines[n0:]), flush=True)
        if args.out:        # written workload by workload: a run that is cut short leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
