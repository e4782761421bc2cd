#!/usr/bin/env python3
"""Per-query tag filters, measured on the SIFT1M-shaped workload bench.py uses (tools/row_filter_bench.py's setup: 10^6 x
128, the learned 16-bit hash of checkpoints/, 10^4 queries, k = 10, 10 probes), one float32 index, ONE query key table for every variant.
GPU only; reads nothing outside the repository.  Two parts:

  1. the tiled scan kernel alone (HIP events around it, `events=`), variants interleaved round by round, the order reversed every other
     round, after an untimed warm-up round; median (min..max), and the ratio to the unfiltered kernel of the same run:
       bscan3_kernel  unfiltered (the parent commit's code: tools/isa_lint.py --compare, profiles/row_tags.txt);
       bscanf_kernel  a RowFilter that allows every row / half of the rows / 1 in 64;
       bscang_kernel  tags against ONE mask for the whole batch that passes every row ("all", mask 0) / half / 1 in 64 of them
                      ("any" on the bits of 32 of the 64 tenants / on one tenant's bit), and 64 distinct tenants dealt over the batch
                      (query i asks for tenant i % 64).  A row's tag is the one bit of its tenant, bit 63 among them.
  2. one `query_tensors` call with the 64 tenants in the batch against the 64 `filter=` calls it replaces (each on the queries of
     one tenant, their RowFilters built beforehand), on the host clock ending in a synchronise.

    python tools/row_tags_bench.py [--rows N] [--queries Q] [--rounds 7] [--iters 10] [--steps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nlsh_amd import io, synth  # noqa: E402
from nlsh_amd.data import SIFT  # noqa: E402
from nlsh_amd.indexer import Indexer  # noqa: E402
from row_filter_bench import K, P, fmt, host_ms, spread  # noqa: E402

TENANTS = 64
HALF_MASK = 0xAAAAAAAAAAAAAAAA   # the odd tenants, tenant 63 (the sign bit of the container) among them


def build(n_rows, Q, dev):
    corpus_h, queries_h = synth.sift_manifold(n_rows, 128, seed=synth.SEED_DATA), synth.sift_manifold(Q, 128, seed=synth.SEED_QUERY)
    Ws, bs = io.load_hasher_weights(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "checkpoints", "sift1m_manifold_h16.npz"))
    Ws, bs = [np.asarray(W, np.float32) for W in Ws], [np.asarray(b, np.float32) for b in bs]
    _, mean, std = synth.standardise(corpus_h)
    Ws[0] = (Ws[0] / std[None, :]).astype(np.float32)
    bs[0] = (bs[0] - Ws[0] @ mean).astype(np.float32)
    rng = np.random.default_rng(3)
    tags = np.uint64(1) << rng.integers(0, TENANTS, size=n_rows).astype(np.uint64)      # one tenant per row, one bit per tenant
    corpus, q = torch.from_numpy(corpus_h).to(dev), torch.from_numpy(queries_h).to(dev)
    ix = Indexer(io.hashing_from_weights(Ws, bs, compat=True), corpus, SIFT.distance, compat=True, algo="tiled",
                 tags=torch.from_numpy(tags.view(np.int64)).to(dev))
    keys, nkeys = ix.hash_device(q, hash_times=P, seed=7)
    return ix, tags, q, keys, nkeys


def scan_ms(ix, q, keys, nkeys, kw, iters):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record(); b.record()
    for ev in evs:
        ix.scan_tensors(q, keys, nkeys, k=K, check=False, events=ev, **kw)
    torch.cuda.synchronize()
    assert int(ix.last_status.cpu()[1]) == 0, "task table overflow inside a timed region"
    return float(np.mean([a.elapsed_time(b) for a, b in evs]))


def same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="scan launches per variant and round")
    ap.add_argument("--steps", type=int, default=5, help="calls per host-clock figure and round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("row_tags_bench needs a GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda", 0)
    ix, tags, q, keys, nkeys = build(args.rows, args.queries, dev)
    N, Q = args.rows, args.queries
    half = (tags & np.uint64(HALF_MASK)) != 0
    one64 = (tags & np.uint64(1)) != 0                                       # tenant 0
    tenant_of_query = torch.arange(Q, device=dev) % TENANTS
    tenant_masks = (torch.ones_like(tenant_of_query) << tenant_of_query).to(torch.int64)
    F = {"all": ix.row_filter(mask=torch.ones(N, dtype=torch.bool, device=dev)), "half": ix.row_filter(mask=torch.from_numpy(half).to(dev)),
         "1/64": ix.row_filter(mask=torch.from_numpy(one64).to(dev))}
    variants = [
        ("bscan3 unfiltered", {}),
        ("bscanf all rows", dict(filter=F["all"])), ("bscanf 1/2", dict(filter=F["half"])), ("bscanf 1/64", dict(filter=F["1/64"])),
        ("bscang all-pass", dict(tag_mask=0, tag_match="all")), ("bscang 1/2", dict(tag_mask=HALF_MASK, tag_match="any")),
        ("bscang 1/64", dict(tag_mask=1, tag_match="any")), ("bscang 64 tenants", dict(tag_mask=tenant_masks, tag_match="any")),
    ]
    ref = ix.scan_tensors(q, keys, nkeys, k=K, want_keys=True)               # sizes the task table
    # what is timed is what is defined: the tagged calls against the filtered ones, word for word
    assert same(ix.scan_tensors(q, keys, nkeys, k=K, want_keys=True, tag_mask=0, tag_match="all"), ref)
    for a, b in (("bscang 1/2", "bscanf 1/2"), ("bscang 1/64", "bscanf 1/64")):
        kw_a, kw_b = dict(variants)[a], dict(variants)[b]
        assert same(ix.scan_tensors(q, keys, nkeys, k=K, want_keys=True, **kw_a), ix.scan_tensors(q, keys, nkeys, k=K, want_keys=True, **kw_b)), a
    lines, res = [], {"N": N, "Q": Q, "k": K, "hash_times": P, "rounds": args.rounds, "n_buckets": ix.n_buckets,
                      "candidates": int(ref[2].long().sum().item()), "rows_half": int(half.sum()), "rows_1_64": int(one64.sum())}
    for _, kw in variants:
        scan_ms(ix, q, keys, nkeys, kw, 3)
    rounds = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, kw in (variants if r % 2 == 0 else variants[::-1]):
            rounds[name].append(scan_ms(ix, q, keys, nkeys, kw, args.iters))
    base = spread(rounds["bscan3 unfiltered"])
    res["scan_ms"] = {name: dict(spread(v), ratio=float(np.median(v)) / base["median"]) for name, v in rounds.items()}
    lines.append(f"sift1m: N={N} d=128 Q={Q} k={K} hash_times={P}, {ix.n_buckets} buckets, {res['candidates']} candidates per batch (before any filter); "
                 f"rows of the 32 odd tenants {res['rows_half']}, rows of tenant 0 {res['rows_1_64']}; {args.rounds} interleaved rounds (order reversed "
                 f"every other round) x {args.iters} scan launches between HIP events, after a warm-up round")
    lines.append(f"  {'variant':20} {'scan ms median (min..max)':>30} {'x unfiltered':>13}")
    for name, r in res["scan_ms"].items():
        lines.append(f"  {name:20} {fmt(r):>30} {r['ratio']:13.3f}")

    # ---- 2. one tagged call against the 64 filtered calls it replaces
    n_t = min(TENANTS, Q)
    per_tenant = []
    for t in range(n_t):
        rows = torch.nonzero(tenant_of_query == t).reshape(-1)
        per_tenant.append((q[rows].contiguous(), ix.row_filter(mask=torch.from_numpy((tags & (np.uint64(1) << np.uint64(t))) != 0).to(dev))))
    one = lambda: ix.query_tensors(q, k=K, hash_times=P, seed=7, tag_mask=tenant_masks, tag_match="any")          # noqa: E731

    def many():
        for qt, Ft in per_tenant:
            ix.query_tensors(qt, k=K, hash_times=P, seed=7, filter=Ft)

    one(); many()
    t_one, t_many = [], []
    for r in range(args.rounds):
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):
            (t_one if which == 0 else t_many).append(host_ms(one if which == 0 else many, args.steps))
    res["tenants"] = {"tenants": n_t, "one_tagged_call_ms": spread(t_one), "filtered_calls_ms": spread(t_many),
                      "ratio": float(np.median(t_many) / np.median(t_one))}
    lines.append(f"{n_t} tenants in one batch of {Q} queries: ONE query_tensors(tag_mask=) call {fmt(res['tenants']['one_tagged_call_ms'])} ms; the "
                 f"{n_t} query_tensors(filter=) calls it replaces, one per tenant on that tenant's queries, filters built beforehand: "
                 f"{fmt(res['tenants']['filtered_calls_ms'])} ms ({res['tenants']['ratio']:.1f}x); host clock ending in a synchronise, "
                 f"{args.rounds} rounds x {args.steps} calls")
    print(json.dumps(res), flush=True)
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
