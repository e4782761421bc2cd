#!/usr/bin/env python3
"""Device time of `nlsh_probe_ranked` alone, beside the encode launch of the same run (profiles/ranked_probes.txt).

    python tools/probe_ranked_bench.py [--rows 10000] [--probes 10,32,128] [--launches 50] [--model checkpoints/sift1m_manifold_h16.npz]

Every figure is the median (min .. max) of `--launches` single launches after a warm-up, each bracketed by a pair of device events
queued behind a short spin kernel (the host runs ahead, so no enqueue gap sits between the events).  z and the hard codes are the encoder's own for `--rows` synthetic SIFT-shaped queries (H = the model's).
Lines: the encode launch the ranked mode makes (one probe, z and code handed out), the sampled mode's encode launch with P probes
(what the ranked mode's two launches replace), `nlsh_probe_ranked` with P probes.  One JSON line per P.
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
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
