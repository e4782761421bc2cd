#!/usr/bin/env python
"""`Indexer.add` / `Indexer.remove` against the rebuild they replace, in ONE process on one box (profiles/index_update.txt).

    python tools/index_update_bench.py [--repeats 20] [--sizes 1,1000,10000,100000] [--out profiles/index_update.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/index_update_bench.py --trace-only --sizes 10000 --repeats 5

Workload: the SIFT1M-shaped index of tools/eval_curve.py (10^6 x 128-d `synth.sift_manifold` rows, the 16-bit hash of
checkpoints/sift1m_manifold_h16.npz, compat=False).  Every timed call starts from the SAME 10^6-row index: a mutation is out of place
and replaces the Indexer's attributes, so the base state is put back (a dict of references, no copy) before each call.
Timed, `--repeats` times each after `--warmup` untimed calls, host clock from a device synchronise to the end of the call (every call
here ends in its own synchronisation: it reads the bucket count back) and, for the library call alone, device events:
  add M / remove M          M in --sizes; added rows are fresh `sift_manifold` rows hashed by the call, removed ids are a random sample
  csr_update M              the `nlsh_csr_update` call of `add M` alone between two device events: all its kernels (sort of the M keys,
                            index pass, bucket table, row pass)
  rebuild                   what the parent commit needs for either: `Indexer(h, torch.cat([corpus, new]))` with M = 10^4 (encode, sort, gather)
  rebuild, keys given       the same with `corpus_keys=`: no encode -- the fair floor of a rebuild
  copy                      `dst.copy_(src)` of a buffer the size of `corpus_sorted`, device events: the bandwidth yardstick
Cache state: steady state of a loop of the same call; the sorted corpus is 512 MB, twice the 256 MiB Infinity Cache, and every call
streams it once, so each call finds at most the tail of the previous pass in cache.
Derived: bytes the row pass moves ((n_kept + M) * row_stride * 4, read + written) over the whole `csr_update` device time -- a LOWER
bound of the row pass's rate, the call's other kernels included -- as a fraction of the copy's rate in the same run.
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


def stats(v):
    a = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)), "min": float(a.min()),
            "max": float(a.max()), "n": int(len(a))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="checkpoints/sift1m_manifold_h16.npz")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--sizes", default="1,1000,10000,100000")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table here")
    ap.add_argument("--trace-only", action="store_true", help="no timing: `--repeats` add calls, then as many remove calls, per size, for a kernel trace of the run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("index_update_bench needs the GPU: nothing here can be timed without one")
    from nlsh_amd import _capi, io as nio, synth
    from nlsh_amd.data import SIFT
    from nlsh_amd.indexer import Indexer

    sizes = [int(s) for s in args.sizes.split(",") if s]
    model = args.model if os.path.exists(args.model) else os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", args.model)
    Ws, bs = nio.load_hasher_weights(model)
    hashing = nio.hashing_from_weights(Ws, bs, compat=False)
    m_max = max(sizes)
    data, mean, std = synth.standardise(synth.sift_manifold(args.n + m_max, 128))
    cg, new = torch.from_numpy(data[:args.n]).cuda(), torch.from_numpy(data[args.n:]).cuda()
    ix = Indexer(hashing, cg, SIFT.distance, compat=False)
    base = dict(ix.__dict__)
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    lines = [f"# index: {args.n} x 128, {ix.bucket_stats()}, repeats={args.repeats}, warmup={args.warmup}, torch {torch.__version__}, "
             f"{torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)

    def restore():
        ix.__dict__.clear()
        ix.__dict__.update(base)

    def host_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def timed(fn, before=restore):
        times = []
        for i in range(args.warmup + args.repeats):
            before()
            dt, out = host_ms(fn)
            del out
            if i >= args.warmup:
                times.append(dt)
        return times

    def emit(row):
        line = json.dumps(row)
        lines.append(line)
        print(line, flush=True)

    if args.trace_only:
        for M in sizes:
            timed(lambda: ix.add(new[:M]))
            gone = torch.from_numpy(rng.choice(args.n, size=M, replace=False).astype(np.int32)).cuda()
            timed(lambda: ix.remove(gone))
            emit({"row": f"add {M}, then remove {M}", "trace_only": True, "calls_each": args.warmup + args.repeats})
        return

    # the yardstick: a copy of a buffer the size of corpus_sorted
    src, dst = ix.corpus_sorted, torch.empty_like(ix.corpus_sorted)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy = []
    for i in range(args.warmup + args.repeats):
        ev0.record()
        dst.copy_(src)
        ev1.record()
        ev1.synchronize()
        if i >= args.warmup:
            copy.append(ev0.elapsed_time(ev1))
    del dst
    copy_bytes = 2 * src.numel() * 4
    copy_rate = copy_bytes / (np.median(copy) * 1e-3)
    emit({"row": "copy", "bytes_read_plus_written": copy_bytes, "device_ms": stats(copy), "TB_per_s": copy_rate / 1e12})

    add_ms = {}
    for M in sizes:
        add_ms[M] = stats(timed(lambda: ix.add(new[:M])))
        emit({"row": f"add {M}", "host_ms": add_ms[M]})
    for M in sizes:
        gone = torch.from_numpy(rng.choice(args.n, size=M, replace=False).astype(np.int32)).cuda()
        emit({"row": f"remove {M}", "host_ms": stats(timed(lambda: ix.remove(gone)))})

    # the library call of `add M` alone, device events around all its kernels
    restore()
    L, stride, N = _capi.lib(), ix.row_stride, args.n
    for M in sizes:
        rows = new[:M]
        keys = ix.hash_device(rows, hash_times=1)[0].reshape(-1).contiguous()
        ids = torch.arange(N, N + M, dtype=torch.int32, device="cuda")
        n_out = N + M
        sorted_out = torch.empty((n_out, stride), dtype=torch.float32, device="cuda")
        gid_out, src_out = (torch.empty((n_out,), dtype=torch.int32, device="cuda") for _ in range(2))
        uniq_out, offs_out = (torch.empty((n_out + 1,), dtype=torch.int32, device="cuda") for _ in range(2))
        nb_out = torch.zeros((1,), dtype=torch.int32, device="cuda")
        wb = L.nlsh_csr_update_workspace(N, ix.n_buckets, M)
        ws = torch.empty((wb,), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        call = []
        for i in range(args.warmup + args.repeats):
            ev0.record()
            _capi.check(L.nlsh_csr_update(_capi.ptr(ix.corpus_sorted), stride, ix.dim, _capi.ptr(ix.gid), None, _capi.ptr(ix.uniq_keys),
                                          _capi.ptr(ix.offsets), N, ix.n_buckets, None, N, _capi.ptr(rows), rows.stride(0), _capi.ptr(keys),
                                          _capi.ptr(ids), M, _capi.ptr(sorted_out), stride, _capi.ptr(gid_out), None, _capi.ptr(src_out),
                                          _capi.ptr(uniq_out), _capi.ptr(offs_out), _capi.ptr(nb_out), _capi.ptr(ws), wb, stream))
            ev1.record()
            ev1.synchronize()
            if i >= args.warmup:
                call.append(ev0.elapsed_time(ev1))
        row_bytes = 2 * n_out * stride * 4
        rate = row_bytes / (np.median(call) * 1e-3)
        emit({"row": f"csr_update {M}", "device_ms": stats(call), "row_pass_bytes": row_bytes, "TB_per_s_lower_bound": rate / 1e12,
              "fraction_of_copy": rate / copy_rate})
        del sorted_out, gid_out, src_out, ws

    # the rebuilds
    M = 10_000 if 10_000 <= m_max else m_max
    keys = torch.cat([ix.corpus_keys, ix.hash_device(new[:M], hash_times=1)[0].reshape(-1)]).contiguous()
    rebuild = stats(timed(lambda: Indexer(hashing, torch.cat([cg, new[:M]]), SIFT.distance, compat=False), before=lambda: None))
    emit({"row": f"rebuild (cat + encode + sort + gather), M={M}", "host_ms": rebuild})
    floor = stats(timed(lambda: Indexer(hashing, torch.cat([cg, new[:M]]), SIFT.distance, compat=False, corpus_keys=keys), before=lambda: None))
    emit({"row": f"rebuild, keys given (cat + sort + gather), M={M}", "host_ms": floor})
    if M in add_ms:
        emit({"row": f"add {M} vs rebuild", "add_over_rebuild": add_ms[M]["median"] / rebuild["median"],
              "add_over_rebuild_keys_given": add_ms[M]["median"] / floor["median"]})
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
