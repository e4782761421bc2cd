#!/usr/bin/env python3
"""Streamed-encoder timing (nlsh_encode_hash_stream, hidden layers > 632): the 1M-row index-build encode and the 10^4-row,
10-probe query batch, for [128,1024,1024,16] and [128,2048,2048,16].  Device events around `hash_device` after a warm-up; FLOPs
from the shapes (2 * sum K*N per row); fraction of the 157.3 TF fp32 MFMA peak.  One JSON line per (encoder, shape), then a summary.
    python tools/enc_wide_bench.py [--reps-build 5] [--reps-query 50] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from nlsh_amd import io, synth  # noqa: E402

PEAK_TF = 157.3
ENCODERS = ([128, 1024, 1024, 16], [128, 2048, 2048, 16])


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps-build", type=int, default=5)
    ap.add_argument("--reps-query", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    x = torch.randn((1_000_000, 128), device="cuda")
    q = x[:10_000].contiguous()
    rows = []
    for dims in ENCODERS:
        Ws, bs = synth.make_weights(dims, seed=1)
        h = io.hashing_from_weights(Ws, bs, compat=True)
        assert h.streamed()
        flop_row = 2.0 * sum(a * b for a, b in zip(dims[:-1], dims[1:]))
        for name, xx, n, n_multi, reps in (("build_1M", x, 1, None, args.reps_build), ("query_10k_p10", q, 10, 8192, args.reps_query)):
            ms = timed(lambda: h.hash_device(xx, n=n, n_multi_rows=n_multi, seed=3), reps)
            tf = flop_row * xx.shape[0] / (ms * 1e-3) / 1e12
            r = dict(encoder=dims, shape=name, rows=xx.shape[0], probes=n, ms=round(ms, 4), mflop_per_row=round(flop_row / 1e6, 3),
                     tflops=round(tf, 2), frac_of_peak=round(tf / PEAK_TF, 3),
                     workspace_mb=round(max(w.numel() for w in h._stream_ws.values()) / 2**20, 1))
            rows.append(r)
            print(json.dumps(r), flush=True)
    summary = dict(tool="enc_wide_bench", peak_tf=PEAK_TF, device=torch.cuda.get_device_name(0), results=rows)
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
