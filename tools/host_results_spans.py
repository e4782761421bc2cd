#!/usr/bin/env python3
"""How long a row range of `Indexer.query()` takes to reach the host after its merge kernel (headline workload).

    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -- python3 bench.py     # a run of its own, no counters
    python3 tools/host_results_spans.py DIR

A row range = the five launches of one `nlsh_query_batch` call (encode_hash ... bmerge) and whatever the facade queues behind them to
bring the range's results to the host.  Per range the table gives, from the trace's device timestamps:
    merge_us        duration of the merge kernel
    copies          device->host copies between the merge's end and the next kernel of the library: records of the memory-copy trace
                    AND the runtime's own copy kernels (`__amd_rocclr_copyBuffer*`: a copy into pinned memory is a blit kernel on this
                    runtime and shows in the kernel trace, not in the copy trace)
    to_last_copy    end of the merge -> end of the last of those copies (0 when there is none)
    to_next_encode  end of the merge -> start of the next range's encode, for ranges whose successor was queued behind them in the SAME call
                    (the second range of a two-range call is followed by host work -- list building -- and is not counted)
Medians over the ranges of the run's steady state (the first `--skip` ranges, warm-up, are left out), plus each figure's quartiles."""
import argparse
import csv
import glob
import gzip
import statistics


def _open(path):
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path)


def load(directory):
    kernels, copies = [], []
    for f in glob.glob(directory + "/**/*kernel_trace.csv*", recursive=True):
        for r in csv.DictReader(_open(f)):
            n = r["Kernel_Name"]
            if "__amd_rocclr_copy" in n:
                copies.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
            elif "nlsh::" in n:
                kernels.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n.split("nlsh::")[1].split("(")[0], int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0)))
    for f in glob.glob(directory + "/**/*memory_copy_trace.csv*", recursive=True):
        for r in csv.DictReader(_open(f)):
            d = r.get("Direction", "")
            if "DEVICE_TO_HOST" in d.upper() or "DTOH" in d.upper():
                copies.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    kernels.sort()
    copies.sort()
    return kernels, copies


def quart(v):
    if len(v) < 2:
        return (v[0],) * 3 if v else (0.0,) * 3
    q = statistics.quantiles(v, n=4)
    return q[0], statistics.median(v), q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("directory")
    ap.add_argument("--skip", type=int, default=8, help="row ranges at the head of the run left out (warm-up calls)")
    ap.add_argument("--same-call-us", type=float, default=150.0, help="a successor that starts within this many us of the merge's end was queued behind it in the same call")
    args = ap.parse_args()
    kernels, copies = load(args.directory)
    merges = [i for i, k in enumerate(kernels) if k[2].startswith("bmerge")]
    if not merges:
        raise SystemExit("no merge kernel in the trace")
    grids = [kernels[i][3] for i in merges]
    grid = max(set(grids), key=grids.count)          # the ranges of the timed calls: the most frequent merge grid
    rows = []
    for i in merges:
        s, e, name, g = kernels[i]
        if g != grid:
            continue
        nxt = kernels[i + 1] if i + 1 < len(kernels) else None
        horizon = nxt[0] if nxt else e + 200_000          # the run's last range: what follows within 0.2 ms
        cs = [c for c in copies if c[0] >= s and c[0] < horizon]
        rows.append(dict(name=name, merge=(e - s) / 1e3, n=len(cs), last=(max(c[1] for c in cs) - e) / 1e3 if cs else 0.0,
                         nxt=(nxt[0] - e) / 1e3 if nxt and nxt[2].startswith("encode_hash") else None))
    rows = rows[args.skip:]
    names = sorted({r["name"] for r in rows})
    print(f"{len(rows)} row ranges (merge grid {grid} work-items, first {args.skip} left out); merge kernel: {', '.join(names)}")
    print(f"device->host copies (copy records + copy kernels) behind a merge: {sorted({r['n'] for r in rows})} per range")
    same = [r["nxt"] for r in rows if r["nxt"] is not None and r["nxt"] < args.same_call_us]
    print("figure                                   ranges   q1_us  median_us   q3_us")
    for label, v in (("merge kernel duration", [r["merge"] for r in rows]),
                     ("merge end -> end of the last copy", [r["last"] for r in rows]),
                     ("merge end -> next range's encode start", same)):
        q1, med, q3 = quart(v)
        print(f"{label:40s} {len(v):6d} {q1:7.1f} {med:10.1f} {q3:7.1f}")


if __name__ == "__main__":
    main()
