#!/usr/bin/env python3
"""Device time of `nlsh_probe_ranked` alone, beside the encode launch of the same run (profiles/ranked_probes.txt), and of
`nlsh_probe_ranked_budget` beside it (profiles/ranked_budget.txt).

    python tools/probe_ranked_bench.py [--rows 10000] [--probes 10,32,128] [--launches 50] [--model checkpoints/sift1m_manifold_h16.npz]
    python tools/probe_ranked_bench.py --budget [--index-rows 1000000] [--keep 10]

Every figure is the median (min .. max) of `--launches` single launches after a warm-up, each bracketed by a pair of device events
queued behind a short spin kernel (the host runs ahead, so no enqueue gap sits between the events).  z and the hard codes are the encoder's own for `--rows` synthetic SIFT-shaped queries (H = the model's).
Lines: the encode launch the ranked mode makes (one probe, z and code handed out), the sampled mode's encode launch with P probes
(what the ranked mode's two launches replace), `nlsh_probe_ranked` with P probes.  One JSON line per P.
--budget: the SIFT1M-shaped index of tools/eval_curve.py is built first (`--index-rows` synthetic rows hashed by the model) and every P
also times `nlsh_probe_ranked_budget` on its CSR arrays with budget = INT32_MAX (every lookup, no early stop) and gives the ratio to
`nlsh_probe_ranked` of the same run; a last line times cap 128 with the budget at which a query keeps `--keep` keys on average (found
by bisection before anything is timed) beside the unbudgeted kernel at P = `--keep` and P = 128.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn, launches, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(200000)          # the device spins while the host queues event, launch, event: no host gap between them
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return {"us_median": round(statistics.median(out), 2), "us_min": round(min(out), 2), "us_max": round(max(out), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="checkpoints/sift1m_manifold_h16.npz")
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--probes", default="10,32,128")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--budget", action="store_true", help="also time nlsh_probe_ranked_budget on the index of --index-rows synthetic rows")
    ap.add_argument("--index-rows", type=int, default=1_000_000)
    ap.add_argument("--keep", type=int, default=10, help="--budget: mean kept keys per query of the early-stop measurement")
    args = ap.parse_args()
    from nlsh_amd import _capi, io as nio, synth
    model = args.model if os.path.exists(args.model) else os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", args.model)
    Ws, bs = nio.load_hasher_weights(model)
    h = nio.hashing_from_weights(Ws, bs, compat=False)
    d, H = h.dims()[0], h.output_dim
    x = torch.from_numpy(synth.standardise(synth.sift_manifold(args.rows, d, seed=synth.SEED_QUERY))[0]).cuda()
    z, _, code = h.forward_device(x)
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    print(f"# {torch.cuda.get_device_name(0)}; {args.rows} rows, dims {h.dims()}; device events around single launches, "
          f"median (min .. max) of {args.launches} after 10 warm-up launches, us", flush=True)
    ix = None
    if args.budget:
        from nlsh_amd.data import SIFT
        from nlsh_amd.indexer import Indexer
        corpus, mean, std = synth.standardise(synth.sift_manifold(args.index_rows, d))
        x = torch.from_numpy(synth.standardise(synth.sift_manifold(args.rows, d, seed=synth.SEED_QUERY), mean, std)[0]).cuda()
        z, _, code = h.forward_device(x)
        ix = Indexer(h, torch.from_numpy(corpus).cuda(), SIFT.distance, compat=False)
        print(f"# index: {ix.bucket_stats()}", flush=True)
    ncand = torch.empty((args.rows,), dtype=torch.int32, device=x.device)

    def budgeted(P, budget, keys, nkeys):
        _capi.check(L.nlsh_probe_ranked_budget(_capi.ptr(z), H, _capi.ptr(code), args.rows, H, h.key_mode, P, args.rows, _capi.ptr(ix.uniq_keys),
                                               _capi.ptr(ix.offsets), ix.n_buckets, budget, _capi.ptr(keys), _capi.ptr(nkeys), None, _capi.ptr(ncand), stream))

    for P in [int(v) for v in args.probes.split(",")]:
        keys = torch.empty((args.rows, P), dtype=torch.int32, device=x.device)
        nkeys = torch.empty((args.rows,), dtype=torch.int32, device=x.device)

        def probe():
            _capi.check(L.nlsh_probe_ranked(_capi.ptr(z), H, _capi.ptr(code), args.rows, H, h.key_mode, P, args.rows,
                                            _capi.ptr(keys), _capi.ptr(nkeys), None, stream))

        rec = {"rows": args.rows, "H": H, "P": P,
               "encode_one_probe_with_z": timed(lambda: h.forward_device(x), args.launches),
               "encode_sampled": timed(lambda: h.hash_device(x, n=P, seed=1, out=(keys, nkeys)), args.launches),
               "probe_ranked": timed(probe, args.launches),
               "hash_device_ranked_two_launches": timed(lambda: h.hash_device(x, n=P, out=(keys, nkeys), probes="ranked"), args.launches)}
        rec["mean_distinct_keys_ranked"] = float(nkeys.float().mean())
        if ix is not None:
            rec["probe_ranked_budget_int32_max"] = timed(lambda: budgeted(P, 0x7FFFFFFF, keys, nkeys), args.launches)
            rec["budget_over_plain"] = round(rec["probe_ranked_budget_int32_max"]["us_median"] / rec["probe_ranked"]["us_median"], 3)
            rec["n_buckets"], rec["mean_candidates"] = ix.n_buckets, float(ncand.float().mean())
        print(json.dumps(rec), flush=True)
    if ix is not None:
        cap = _capi.MAX_ENCODE_PROBES
        keys = torch.empty((args.rows, cap), dtype=torch.int32, device=x.device)
        nkeys = torch.empty((args.rows,), dtype=torch.int32, device=x.device)
        lo, hi = 1, 0x7FFFFFFF                   # the smallest budget at which a query keeps >= --keep keys on average
        while lo < hi:
            mid = (lo + hi) // 2
            budgeted(cap, mid, keys, nkeys)
            lo, hi = (lo, mid) if float(nkeys.float().mean()) >= args.keep else (mid + 1, hi)
        budgeted(cap, lo, keys, nkeys)
        rec = {"rows": args.rows, "H": H, "cap": cap, "budget": lo, "mean_kept_keys": float(nkeys.float().mean()),
               "median_kept_keys": float(nkeys.float().median()), "max_kept_keys": int(nkeys.max()), "mean_candidates": float(ncand.float().mean()),
               "probe_ranked_budget_cap128": timed(lambda: budgeted(cap, lo, keys, nkeys), args.launches)}
        for P in (args.keep, cap):
            rec[f"probe_ranked_P{P}"] = timed(lambda: _capi.check(L.nlsh_probe_ranked(
                _capi.ptr(z), H, _capi.ptr(code), args.rows, H, h.key_mode, P, args.rows, _capi.ptr(keys), _capi.ptr(nkeys), None, stream)), args.launches)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
