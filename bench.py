#!/usr/bin/env python3
"""Headline benchmark: queries/sec + recall@10 of the nlsh query-time hot path on MI355X.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment starts the N ranks itself (a torchrun child
process, before this process touches the GPU) and exits with its code; a WORLD_SIZE that disagrees with --gpus is an
error, never a silent 1-GPU run.

Workload = BASELINE.json configs[1]: SIFT1M-shaped, 1M x 128-d corpus, 10k queries per batch, 16-bit learned hash,
k=10, hash_times=10.  A "step" = ONE `Indexer.query(batch, k=10, hash_times=10)` call -- the reference's QPS protocol
(nlsh/trainers/base.py:93-96,107-108): queries already in HBM, index built, hashing included, and
the call returns the reference's Python lists (so it ends with the device->host copy of the ids).  K such calls are
timed between barrier + synchronize pairs, rotating over `--batches` different query batches:
    value        = Q * K / elapsed            (whole job, max over ranks)
    ms_per_step  = elapsed / K
The same hot path with results LEFT IN HBM (`query_tensors`: encode_hash -> plan -> scan -> merge, what a serving
pipeline that consumes device tensors sees) is timed in a second K-step region and reported as the top-level fields
`device_resident_qps` / `device_resident_ms_per_step`; its scan kernel is bracketed by HIP events on the launch
stream, which is where `roofline` comes from.  At N=1 the kernels of a device-resident step run back to back on one
stream (each kernel alone on the chip: ONE `nlsh_query_batch` call, five launches); at N>1 they go through the graph slots of
nlsh_amd/pipeline.py with the all-gather behind each batch on its slot's stream (`--pipeline on|off` forces either), and the scan
kernel is timed alone in a short sequential region of its own.  The `--full` N=1 run also carries `workloads`: configs[2]
(GloVe-1.2M-shaped) and configs[1] on SURVEY 8(d)'s own generator, 3 + 20 device-resident steps each (`--no-side-workloads` skips).
N>1: corpus buckets sharded over the ranks (whole buckets per rank, one build-time all-to-all; `--shard rows` keeps
contiguous row ranges), every rank answers all queries over its shard, one all-gather (RCCL) of the per-rank top-k +
merge per step ("strong" scaling: total work fixed).

A plain run measures the headline alone: set up, build the index, warm up, time the K protocol steps, write the last step's lists
if `--dump-outputs DIR` is given (DIR/ids.npy, n_candidates.npy, query_rows.npy; fixed probe seeds, so the same arguments give the
same arrays), compute recall@10 with one more call and print the line.  Everything else described here -- index rebuild time,
`protocol_qps_opt_in`, `own_slice_qps`, the device-resident region and `roofline`, the folded-L2 and pipelined regions, `encoder`,
`cpu_baseline`, `workloads` -- is measured with `--full` only.

`value` is measured with the facade's DEFAULT settings (what an unmodified Trainer.fit gets); `protocol_qps_opt_in` is the
same region with the two host-side opt-ins.  `--l2-form folded` prints the complete line on the opt-in
2-op L2 form instead (config.l2_form).

`roofline`: the query-major schedule re-reads every row per query: bound = "hbm", achieved = 4*d*sum(C_q) B / kernel
time against 8 TB/s.  The bucket-major schedules share a fetched row between the queries of a group, so two roofs can bind
them, both on algorithmic quantities measured live: pair flops (3*d*sum(C_q), 2*d for cosine) against the 157.3 TF fp32
vector peak, and the bytes of the batch's DISTINCT candidate rows against 8 TB/s; bound = "valu" unless the HBM fraction
exceeds 1.5x the VALU fraction; both fractions are always printed, SURVEY 8(d)'s per-pair byte rate as
`algorithmic_GBps`.  `traffic` = HBM bytes per launch from the committed rocprofv3 --pmc pass of the SAME workload, schedule,
row window and kernel sources (profiles/traffic_r06.json), else null.  `cpu_baseline` = the CPU restatements timed on this
box's host cores on a bounded sample.
There is no dataset or reference checkpoint offline: data is seeded synthetic (`synth.sift_manifold`) and the hash is
the one our minimal trainer learned on it (checkpoints/, see config.hash).
"""
import argparse
import copy
import json
import os
import socket
import subprocess
import sys
import time

# multi-process GPU work on this pool needs dmabuf IPC (the image exports it already; a bare launcher environment may not)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 64 FLOP/clk/SIMD (155 TF measured)
VALU_F32_PEAK_TFLOPS = 157.3  # same figure: 1024 SIMDs x 2.4 GHz x 64 lanes x 2 flop / 2 cycles per wave64 v_fma_f32
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "traffic_r06.json")
KERNEL_SOURCES = ("scan_bucket.hip", "scan_common.h", "scan_topk.hip", "common.h", "build_csr.hip")   # build_csr.hip: the cell packing shapes the scan's tasks


def kernel_source_hash():
    """sha256 over the scan kernels' sources: the committed PMC figures (TRAFFIC_FILE) carry the hash of the code they were
    measured on and are reported only while it still matches the tree (tools/make_traffic.py writes it)."""
    import hashlib
    h = hashlib.sha256()
    for name in KERNEL_SOURCES:
        with open(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "csrc", name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="sift1m", choices=["sift1m", "glove"],
                    help="sift1m = BASELINE.json configs[1] (headline); glove = configs[2] (1,183,514 x 100-d, cosine, 24-bit)")
    ap.add_argument("--data", default="manifold", choices=["manifold", "clusters"],
                    help="sift1m only.  manifold: synth.sift_manifold (6-d latent manifold: nearest neighbours are meaningful, what the "
                         "learned hash is trained on; headline).  clusters: SURVEY 8(d)'s own generator, synth.sift_like (1,000 isotropic "
                         "Gaussian clusters, sigma 24), with the hash trained on it (checkpoints/sift1m_clusters_h16.npz)")
    ap.add_argument("--dataset", default=None,
                    help="REAL data instead of the seeded generators: an ann-benchmarks HDF5 file (needs h5py) or a TEXMEX directory "
                         "(*base.fvecs|bvecs, *query.fvecs, *groundtruth.ivecs), read by nlsh_amd.data.SIFT / Glove (--workload picks the class "
                         "and metric); corpus = `train`, one query batch = the first --queries rows of `test`, recall against the file's own "
                         "`neighbors`.  `data` then reads \"real\".  Pair with --hash-checkpoint (else a random-init hash)")
    ap.add_argument("--hash-checkpoint", default=None, help="hasher weights for --dataset: our .npz, a state dict, or the reference's TorchScript _cpu.pt (nlsh/hashings.py:53-57)")
    ap.add_argument("--unit-norm", action="store_true", help="--dataset: standardise with the training set's mean / std like SIFT(unit_norm=True) (nlsh/data.py:125-129)")
    ap.add_argument("--rows", "--n", dest="n", type=int, default=int(os.environ.get("NLSH_BENCH_N", 0)))
    ap.add_argument("--queries", "--q", dest="q", type=int, default=int(os.environ.get("NLSH_BENCH_Q", 10_000)))
    ap.add_argument("--batches", type=int, default=4, help="distinct query batches the timed steps rotate over")
    ap.add_argument("--dim", type=int, default=0)
    ap.add_argument("--hash-size", type=int, default=0)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--hash-times", type=int, default=10)
    ap.add_argument("--seg-rows", type=int, default=0)
    ap.add_argument("--shard", default="buckets", choices=["buckets", "rows"],
                    help="N>1 partition of the corpus: whole buckets per rank (default) or contiguous row ranges")
    ap.add_argument("--query-chunks", type=int, default=None, help="row ranges Indexer.query() scans a batch in (default: the facade's, 2); 1 for profiling runs: every scan launch of the process then has the full-batch grid and per-kernel-NAME statistics mean one thing")
    ap.add_argument("--pipeline", default="auto", choices=["auto", "on", "off"],
                    help="device-resident region only.  on: three-stage pipeline over three HIP streams; off: every kernel of a "
                         "step back to back on one stream (each kernel alone on the chip); auto: on for N>1, off for N=1")
    ap.add_argument("--algo", default=None, choices=["query", "bucket", "tiled"], help="force a scan schedule (default: auto)")
    ap.add_argument("--window", type=int, default=None, help="row window of the tiled schedule's small-bucket packing (default: the facade's choice, 64; 0 = one task list per bucket)")
    ap.add_argument("--l2-form", default="exact", choices=["exact", "folded"],
                    help="exact (default): sqrt(sum(((q - c) + 1e-6)^2)) in F.pairwise_distance's operation order, bit-identical to the oracle.  folded: the "
                         "WHOLE line (value, roofline, recall) is measured with Indexer(l2_form='folded') = NLSH_METRIC_L2_EPS_FOLDED, "
                         "sqrt(sum(((q + 1e-6) - c)^2)): inside BASELINE.json's 1e-4 tolerance, not the oracle's bits; config.l2_form says so")
    ap.add_argument("--exchange", default="auto", choices=["auto", "allgather"],
                    help="N>1, bucket shards: how rows reach their bucket's owner at index build.  auto: one all_to_all_single with uneven splits "
                         "(probed first, agreed by all ranks); allgather: all-gather + local selection (the fallback, selectable so that a first "
                         "contact with a fabric that refuses uneven all-to-all does not cost the run)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-side-workloads", action="store_true", help="skip the `workloads` object (configs[2] and SURVEY 8(d)'s generator, 3 + 20 device-resident steps each) of the default run")
    ap.add_argument("--random-init", action="store_true", help="ignore the learned-hash checkpoint")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target CPU time of each baseline sample")
    ap.add_argument("--rehearse-launch", action="store_true",
                    help="launch check only (no GPU needed): start the ranks, rendezvous over gloo, print {n_gpus} and exit")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: index rebuild time, the opt-in and own-slice protocol regions, the device-resident "
                         "region with its roofline, the folded-L2 and pipelined regions, encoder / HBM copy figures, cpu_baseline and the "
                         "`workloads` object.  Off: set up, warm up, time --steps protocol steps, recall@10, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the LAST timed step returned to its caller as DIR/*.npy (float64): "
                         "ids.npy [Q, k] (-1 past a short list), n_candidates.npy [Q], query_rows.npy [Q] (rows of the step's batch; a fixed, "
                         "seeded sample of them when the whole would exceed 64 MB)")
    return ap.parse_args(argv)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, ids, ncand, k):
    """The lists `Indexer.query` returned in the last timed step, as float64 arrays: the step's batch and probe seed are fixed, so two
    builds given the same arguments can be compared array for array."""
    Q = len(ids)
    rows = np.arange(Q)
    per_row = 8 * (k + 2)                                   # ids, n_candidates and query_rows
    if Q * per_row > DUMP_LIMIT_BYTES:
        rows = np.sort(np.random.default_rng(0).choice(Q, DUMP_LIMIT_BYTES // per_row, replace=False))
    out = np.full((len(rows), k), -1.0)
    for j, r in enumerate(rows.tolist()):
        out[j, :len(ids[r])] = ids[r]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "ids.npy"), out)
    np.save(os.path.join(out_dir, "n_candidates.npy"), np.asarray(ncand, dtype=np.float64)[rows])
    np.save(os.path.join(out_dir, "query_rows.npy"), rows.astype(np.float64))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args):
    """--gpus N > 1 without a launcher: run the N ranks as a torchrun child (this process has made no GPU call)."""
    # torchrun's own parser prefix-matches options that FOLLOW the script path (`--n` reads as an ambiguous --nnodes /
    # --nproc-per-node): hand the short spellings over in their long form
    long_form = {"--n": "--rows", "--q": "--queries"}
    argv = [long_form.get(a, a) for a in sys.argv[1:]]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + argv
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def collective_facts(world, dev, gpus):
    """What the N>1 line says about the exchange it ran, OBSERVED through the data backend itself: the backend's
    name, the number of ranks an all-reduce of ones saw, and the number of distinct devices among the ranks (all-gather of each rank's
    PCI identity; 1 on the one-GPU rehearsals, N on a real node).  A line whose collective did not see --gpus ranks is never printed."""
    if world == 1:
        return None
    backend = dist.get_backend()
    on = dev if backend == "nccl" else torch.device("cpu")       # gloo rehearsals exchange host tensors
    seen = torch.ones((1,), dtype=torch.int64, device=on)
    dist.all_reduce(seen)
    props = torch.cuda.get_device_properties(dev)
    ident = (int(getattr(props, "pci_domain_id", 0)) << 32) | (int(getattr(props, "pci_bus_id", 0)) << 8) | int(getattr(props, "pci_device_id", 0))
    ident = (ident << 8) | (dev.index & 0xFF)
    mine = torch.tensor([ident], dtype=torch.int64, device=on)
    table = torch.empty((world,), dtype=torch.int64, device=on)
    dist.all_gather_into_tensor(table, mine)
    facts = {"backend": backend + (" (RCCL)" if backend == "nccl" else ""), "world_size_seen": int(seen.item()),
             "distinct_devices": int(torch.unique(table).numel()), "data_tensors_on": on.type}
    if facts["world_size_seen"] != gpus:
        print(f"[bench] the {backend} all-reduce saw {facts['world_size_seen']} ranks, --gpus says {gpus}: refusing to print a line", file=sys.stderr)
        sys.exit(2)
    return facts


def traffic_entry(key, shape, learned):
    """(traffic bytes per launch, VALU wave-instructions per launch, clock held, source note) of the committed rocprofv3 --pmc pass
    whose workload shape, schedule, row window AND kernel source hash equal this run's; Nones otherwise (a kernel change without a
    new PMC pass nulls them instead of quoting stale counters)."""
    try:
        tr = json.load(open(TRAFFIC_FILE))
        ent = tr["entries"].get(key)
        if ent is not None and learned and tr.get("kernel_source_sha256") == kernel_source_hash():
            w = ent["workload"]
            if (w["N"], w["d"], w["Q"], w["H"], w["hash_times"], w["algo"], w["window_rows"]) == tuple(shape):
                src = "profiles/" + os.path.basename(TRAFFIC_FILE) + " (rocprofv3 --pmc on the profile box, same workload, schedule and kernel sources; not this run)"
                return ent["traffic_bytes_per_launch"], ent.get("valu_wave_instructions_per_launch"), ent.get("clock_held_GHz"), src, ent.get("origin")
    except (OSError, KeyError, ValueError, TypeError):
        pass
    return None, None, None, None, None


def batch_sums(indexer, q, k, P, seed):
    """(sum of the batch's candidate counts, rows of the buckets the batch probes at all -- each counted ONCE: what a schedule that shares
    a fetched row between the queries probing its bucket has to read at least) of one batch, by an untimed recomputation."""
    dev = q.device
    sum_c = int(indexer.query_tensors(q, k=k, hash_times=P, seed=seed)[2].long().sum().item())
    uniq_rows = None
    if indexer.n_buckets:
        bucket_rows = (indexer.offsets[1:] - indexer.offsets[:-1]).long()
        kk, nn = indexer.hash_device(q, hash_times=P, seed=seed)
        pos = torch.searchsorted(indexer.uniq_keys, kk.clamp(min=int(indexer.uniq_keys[0]), max=int(indexer.uniq_keys[-1]))).clamp(max=indexer.n_buckets - 1)
        hit = (indexer.uniq_keys[pos] == kk) & (torch.arange(kk.shape[1], device=dev)[None, :] < nn[:, None])
        uniq_rows = int(bucket_rows[torch.unique(pos[hit])].sum().item())
    return sum_c, uniq_rows


def bucket_major_roofline(kernel, metric, d, sum_c, uniq_rows, t_scan):
    """The two roofs of a bucket-major schedule, both on algorithmic quantities measured live: pair flops against the fp32
    vector peak, bytes of the batch's DISTINCT candidate rows against the HBM peak; bound = "valu" unless the HBM fraction is more
    than 1.5x the VALU fraction."""
    algo_flops = (3.0 * d if metric == "l2" else 2.0 * d) * sum_c      # (q-c), +eps, fma per element | one fma
    unique_bytes = 4.0 * d * uniq_rows
    valu_frac = algo_flops / t_scan / 1e12 / VALU_F32_PEAK_TFLOPS
    hbm_frac = unique_bytes / t_scan / 1e9 / HBM_PEAK_GBPS
    if 1.5 * valu_frac >= hbm_frac:
        roof = {"bound": "valu", "kernel": kernel, "achieved": algo_flops / t_scan / 1e12, "peak": VALU_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": valu_frac}
    else:
        roof = {"bound": "hbm", "kernel": kernel, "achieved": unique_bytes / t_scan / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": hbm_frac}
    roof.update({"valu_frac": valu_frac, "hbm_frac_of_distinct_candidate_rows": hbm_frac, "distinct_candidate_row_bytes_per_launch": unique_bytes})
    return roof


SIDE_WORKLOADS = {
    "glove": dict(workload="glove", data="manifold", N=1_183_514, d=100, H=24, metric="cosine", ckpt="glove_manifold_h24.npz",
                  cfg="configs[2]: GloVe-1.2M-shaped (synth.glove_manifold, cosine, 24-bit full-width keys)"),
    "clusters": dict(workload="sift1m", data="clusters", N=1_000_000, d=128, H=16, metric="l2", ckpt="sift1m_clusters_h16.npz",
                     cfg="configs[1] on SURVEY 8(d)'s generator (synth.sift_like: 1,000 isotropic Gaussian clusters, sigma 24, standardised)"),
}


def side_workload(tag, args, dev, steps=20, warmup=3):
    """One of the non-headline workloads inside the DEFAULT run: the code paths of `--workload glove` /
    `--data clusters` -- learned hash from checkpoints/, `Indexer.query_tensors` steps back to back on one stream, the scan kernel
    bracketed by HIP events on its launch stream -- 3 warm-up + 20 timed steps, no protocol region and no CPU leg.  The QPS protocol
    is the reference's (nlsh/trainers/base.py:93-108) with the results left in HBM."""
    from nlsh_amd import _capi, synth
    from nlsh_amd.data import Glove, SIFT, brute_force_topk
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.hashings import MultivariateBernoulli
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.metrics import calculate_recall
    w = SIDE_WORKLOADS[tag]
    N, d, H, metric, Q, k, P, B = w["N"], w["d"], w["H"], w["metric"], args.q, args.k, args.hash_times, 4
    if w["workload"] == "glove":
        corpus_h = synth.glove_manifold(N, d, seed=synth.SEED_DATA)
        batches_h = [synth.glove_manifold(Q, d, seed=synth.SEED_QUERY + 17 * i) for i in range(B)]
    else:
        corpus_h, mean, std = synth.standardise(synth.sift_like(N, d, seed=synth.SEED_DATA))
        batches_h = [synth.standardise(synth.sift_like(Q, d, seed=synth.SEED_QUERY + 17 * i), mean, std)[0] for i in range(B)]
    arrs = np.load(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "checkpoints", w["ckpt"]))
    Ws, bs = [arrs[f"W{i}"] for i in range(3)], [arrs[f"b{i}"] for i in range(3)]
    hashing = MultivariateBernoulli(MultiLayerRelu(d, [256, 256], with_bias=True), H, None, compat=H <= 16)
    lin = [m for m in hashing._hasher.modules() if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, W, b in zip(lin, Ws, bs):
            m.weight.copy_(torch.from_numpy(np.asarray(W, dtype=np.float32)))
            m.bias.copy_(torch.from_numpy(np.asarray(b, dtype=np.float32)))
    hashing.train_mode(False)
    corpus = torch.from_numpy(corpus_h).to(dev)
    qb = [torch.from_numpy(b).to(dev) for b in batches_h]
    indexer = Indexer(hashing, corpus, SIFT.distance if metric == "l2" else Glove.distance, compat=H <= 16)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record(); b.record()
    indexer.query_tensors(qb[0], k=k, hash_times=P, seed=999)           # sizes the task table (checked call), untimed
    for i in range(warmup):
        indexer.query_tensors(qb[i % B], k=k, hash_times=P, seed=1000 + i, check=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        indexer.query_tensors(qb[i % B], k=k, hash_times=P, seed=1000 + i, check=False, events=ev[i])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    n_tasks, overflow = (int(v) for v in indexer.last_status.cpu())
    assert overflow == 0, f"{tag}: task table overflow inside the timed region"
    scan_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    sums = [batch_sums(indexer, qb[i % B], k, P, 1000 + i) for i in range(steps)]
    sum_c, uniq_rows = float(np.mean([s_[0] for s_ in sums])), float(np.mean([s_[1] for s_ in sums]))
    algo = int(indexer.last_algo)
    kernel = {0: "scan_kernel (query-major)", 1: "bscan2_kernel (bucket-major, 8 queries in registers)", 2: "bscan3_kernel (bucket-major, LDS-tiled)"}[algo] + " " + metric
    roof = bucket_major_roofline(kernel, metric, d, sum_c, uniq_rows, scan_ms * 1e-3)
    traffic, _, _, src, dram = traffic_entry(f"{w['workload']}:{w['data']}:exact", (N, d, Q, H, P, algo, int(indexer.last_window)), True)
    roof.update({"traffic": traffic, "traffic_source": src, "avg_launch_ms": scan_ms, "tasks_per_launch": n_tasks})
    if dram is not None:      # DRAM vs Infinity Cache, as far as the pool's counters go (profiles/traffic_r06.json: `origin`)
        roof["traffic_origin"] = dram
    gt = brute_force_topk(qb[0], corpus, k, metric).cpu().numpy()
    ids0, nc0 = indexer.query(qb[0], k=k, hash_times=P, seed=5000)
    stats = indexer.bucket_stats()
    out = {"workload": f"{w['cfg']}, N={N} d={d} Q={Q} H={H} k={k} hash_times={P}, {B} query batches in rotation",
           "hash": f"learned (checkpoints/{w['ckpt']})", "steps": steps, "warmup": warmup,
           "scan_ms": scan_ms, "device_resident_ms_per_step": 1e3 * el / steps, "device_resident_qps": Q * steps / el,
           "recall_at_10": float(np.mean(calculate_recall(list(gt), ids0))), "mean_candidates_per_query": float(np.mean(nc0)),
           "n_buckets": stats["n_indexes"], "window_rows": int(indexer.last_window), "roofline": roof}
    del indexer, corpus, qb
    torch.cuda.empty_cache()
    return out


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world != args.gpus:
        print(f"[bench] WORLD_SIZE={world} disagrees with --gpus={args.gpus}: refusing to report a {world}-rank run as "
              f"{args.gpus} GPUs", file=sys.stderr)
        sys.exit(2)
    if args.rehearse_launch:
        if world > 1:
            dist.init_process_group("gloo")
        seen = torch.ones((1,), dtype=torch.int64)
        if world > 1:
            dist.all_reduce(seen)
        if rank == 0:
            print(json.dumps({"rehearse_launch": True, "n_gpus": world, "ranks_seen": int(seen.item())}), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    if args.exchange == "allgather":
        os.environ["NLSH_SHARD_EXCHANGE"] = "allgather"
    if os.environ.get("NLSH_BENCH_SAME_DEVICE"):  # rehearsal of the N>1 path on a one-GPU box (gloo, all ranks on cuda:0)
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        backend = os.environ.get("NLSH_BENCH_BACKEND", "nccl")  # "nccl" is RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    collective = collective_facts(world, dev, args.gpus)

    from nlsh_amd import _capi, synth
    from nlsh_amd.data import Glove, SIFT, brute_force_topk
    from nlsh_amd.distributed import ShardedIndexer, TopkExchange, gather_and_merge, shard_range
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.hashings import MultivariateBernoulli
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.metrics import calculate_recall
    _capi.lib()  # fail loudly if the HIP library is missing

    wl = {"sift1m": dict(N=1_000_000, d=128, H=16, metric="l2", ckpt="sift1m_manifold_h16.npz", cfg="configs[1]: SIFT1M-shaped "
                         "(synthetic SIFT-like integers on a 6-d latent manifold, synth.sift_manifold, standardised)"),
          "glove": dict(N=1_183_514, d=100, H=24, metric="cosine", ckpt="glove_manifold_h24.npz", cfg="configs[2]: GloVe-1.2M-shaped "
                        "(synthetic 100-d embeddings on an 8-d latent manifold, synth.glove_manifold, cosine)")}[args.workload]
    if args.workload == "sift1m" and args.data == "clusters":
        wl = dict(wl, ckpt="sift1m_clusters_h16.npz", cfg="configs[1]: SIFT1M-shaped (SURVEY 8(d) generator: synthetic SIFT-like integers, "
                  "1,000 isotropic Gaussian clusters, sigma 24, synth.sift_like, standardised)")
    gt_file = None
    if args.dataset:
        # real files: the dataset classes of the facade read them exactly like the reference's (nlsh/data.py:14-46,112-140)
        from nlsh_amd import io as nio
        ds = (SIFT if wl["metric"] == "l2" else Glove)(args.dataset, unit_norm=args.unit_norm)
        ds.load()
        corpus_h = np.ascontiguousarray(ds.training[: args.n] if args.n else ds.training, dtype=np.float32)
        N, d = corpus_h.shape
        Q = min(args.q, ds.testing.shape[0])
        batches_h = [np.ascontiguousarray(ds.testing[:Q], dtype=np.float32)]
        gt_file = np.asarray(ds.ground_truth)[:Q]
        if args.n and gt_file.max() >= N:
            gt_file = None                      # a truncated corpus has other neighbours: brute force below instead
        wl = dict(wl, cfg=f"REAL data {os.path.basename(os.path.normpath(args.dataset))} ({ds.__class__.__name__}, unit_norm={args.unit_norm})")
        if args.hash_checkpoint:
            Ws, bs = nio.load_hasher_weights(args.hash_checkpoint)
            H = int(Ws[-1].shape[0])
            hidden = [int(w.shape[0]) for w in Ws[:-1]]
            hash_desc = f"learned: {args.hash_checkpoint}, {d}->{'->'.join(map(str, hidden))}->{H}"
        else:
            H = args.hash_size or wl["H"]
            hidden = [256, 256]
            Ws, bs = synth.make_weights([d] + hidden + [H], seed=synth.SEED_WEIGHTS)
            hash_desc = f"seeded nn.Linear-default init {d}->256->256->{H} (random-init hash)"
        args.hash_size_eff = H
        k, P, metric, B = args.k, args.hash_times, wl["metric"], 1
    else:
        hidden = [256, 256]
        N, d, H = args.n or wl["N"], args.dim or wl["d"], args.hash_size or wl["H"]
        args.hash_size_eff = H
        Q, k, P, metric, B = args.q, args.k, args.hash_times, wl["metric"], max(1, args.batches)
        if args.workload == "sift1m":
            gen = synth.sift_manifold if args.data == "manifold" else synth.sift_like
            corpus_h, mean, std = synth.standardise(gen(N, d, seed=synth.SEED_DATA))
            batches_h = [synth.standardise(gen(Q, d, seed=synth.SEED_QUERY + 17 * i), mean, std)[0] for i in range(B)]
        else:
            corpus_h = synth.glove_manifold(N, d, seed=synth.SEED_DATA)
            batches_h = [synth.glove_manifold(Q, d, seed=synth.SEED_QUERY + 17 * i) for i in range(B)]
        ckpt = os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "checkpoints", wl["ckpt"])
        if d == wl["d"] and H == wl["H"] and os.path.exists(ckpt) and not args.random_init:
            arrs = np.load(ckpt)
            Ws, bs = [arrs[f"W{i}"] for i in range(3)], [arrs[f"b{i}"] for i in range(3)]
            hash_desc = (f"learned: triplet loss (margin 1.0, random negatives, 5000 Adam steps, tools/train_hash.py) on this "
                         f"synthetic corpus, {d}->256->256->{H}, checkpoints/{wl['ckpt']}")
        else:
            Ws, bs = synth.make_weights([d, 256, 256, H], seed=synth.SEED_WEIGHTS)
            hash_desc = f"seeded nn.Linear-default init {d}->256->256->{H} (random-init hash)"
    # keys wrap to int16 like the reference (nlsh/utils.pyx:7-15) up to 16 bits; wider hashes use the full code
    hashing = MultivariateBernoulli(MultiLayerRelu(d, hidden, with_bias=bs[0] is not None), H, None, compat=H <= 16)
    lin = [m for m in hashing._hasher.modules() if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, W, b in zip(lin, Ws, bs):
            m.weight.copy_(torch.from_numpy(np.asarray(W, dtype=np.float32)))
            if b is not None:
                m.bias.copy_(torch.from_numpy(np.asarray(b, dtype=np.float32)))
    hashing.train_mode(False)

    lo, hi = shard_range(N, rank, world)
    shard = torch.from_numpy(corpus_h[lo:hi]).to(dev)
    qb = [torch.from_numpy(b).to(dev) for b in batches_h]      # inputs resident in HBM before any timed region
    torch.cuda.synchronize()
    t0 = time.time()
    distance = SIFT.distance if metric == "l2" else Glove.distance
    sharded = None
    if world > 1:   # build-time exchange (all-gather of keys + all-to-all of rows for --shard buckets) is inside build_s
        sharded = ShardedIndexer(hashing, shard, distance, id_base=lo, shard=args.shard, compat=H <= 16,
                                 seg_rows=args.seg_rows, algo=args.algo, l2_form=args.l2_form, window_rows=args.window)
        indexer = sharded.local
    else:
        indexer = Indexer(hashing, shard, distance, compat=H <= 16, seg_rows=args.seg_rows, algo=args.algo, l2_form=args.l2_form,
                          window_rows=args.window)
    torch.cuda.synchronize()
    build_s = time.time() - t0
    rebuild_s = None
    if world == 1 and args.full:      # the build that recurs (the reference rebuilds every 300 training steps, main.py:402): allocator warm
        t0 = time.time()
        Indexer(hashing, shard, distance, compat=H <= 16, seg_rows=args.seg_rows, algo=args.algo, l2_form=args.l2_form, window_rows=args.window)
        torch.cuda.synchronize()
        rebuild_s = time.time() - t0
    if args.query_chunks is not None:
        Indexer.query_chunks = max(1, args.query_chunks)
    stats = indexer.bucket_stats()
    steps, warmup = args.steps, args.warmup

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    # ------------------------------------------------------------------ region A: the reference's protocol (headline)
    # `value`: every call returns ALL Q result lists to the calling rank, at every N (the reference's deliverable,
    # nlsh/trainers/base.py:93-96), with the facade's DEFAULTS -- what an unmodified `Trainer.fit` gets.  The same region with the
    # facade's host-side opt-ins on (`Indexer.defer_result_release`, `Indexer.untracked_results`: INTEGRATION.md) is reported beside it
    # as `protocol_qps_opt_in`, and at N>1 the variant in which rank r only builds the lists of its Q/N slice (`own_slice_qps`).
    def protocol_region(own, opt_in):
        saved = (Indexer.defer_result_release, Indexer.untracked_results)
        Indexer.defer_result_release = Indexer.untracked_results = bool(opt_in)
        try:
            def query_lists(i):
                # the step's probe seed is fixed (the same on every rank): the last step's lists are the same from run to run
                if sharded is not None:
                    return sharded.query(qb[i % B], k=k, hash_times=P, seed=5000 + i, own_slice=own)
                return indexer.query(qb[i % B], k=k, hash_times=P, seed=5000 + i)

            held = None
            for i in range(max(warmup, 1)):        # at least one: sizes the task table (may retry once); untimed
                held = query_lists(-1 - i)         # held like the timed loop holds them: the previous call's lists die when the next arrive
            fence()
            calls = []
            t0 = time.perf_counter()
            for i in range(steps):
                t1 = time.perf_counter()
                held = query_lists(i)
                calls.append(time.perf_counter() - t1)
            fence()
            el = max_over_ranks(time.perf_counter() - t0)
            return el, calls, held
        finally:
            Indexer.defer_result_release, Indexer.untracked_results = saved

    elapsed, call_s, (ids_api, nc_api) = protocol_region(own=False, opt_in=False)
    assert isinstance(ids_api, list) and len(ids_api) == Q and isinstance(nc_api, list)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ids_api, nc_api, k)
    elapsed_opt_in, elapsed_own = None, None
    if args.full:
        elapsed_opt_in, _, _ = protocol_region(own=False, opt_in=True)
    if args.full and sharded is not None:
        elapsed_own, _, (ids_own, _) = protocol_region(own=True, opt_in=False)
        q_lo, q_hi = shard_range(Q, rank, world)
        assert len(ids_own) == q_hi - q_lo

    # ------------------------------------------------------------------ --full: everything beside the headline
    if args.full:
        # ------------------------------------------------------------------ region B: same path, results left in HBM
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        ev_x = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for a, b in ev + ev_x:  # instantiate the hipEvent handles
            a.record(); b.record()
        xchg = TopkExchange(k) if world > 1 else None
        cur = [None]

        def exchange(k64, nc):   # tail stage on a sharded index: all-gather of per-shard top-k + merge
            i = cur[0]
            if i is not None:
                ev_x[i][0].record()
            out_ = xchg(k64, nc)
            if i is not None:
                ev_x[i][1].record()
            return out_

        use_pipeline = args.pipeline == "on" or (args.pipeline == "auto" and world > 1)
        pipe = None
        if use_pipeline:
            from nlsh_amd.pipeline import QueryPipeline
            pipe = QueryPipeline(indexer, qb[0], k=k, hash_times=P, depth=3, exchange=exchange if world > 1 else None)

        def device_step(i, events=None, mark=False):
            q = qb[i % B]
            seed = 1000 + i  # identical on every rank -> identical multi-probe keys
            if pipe is not None:
                cur[0] = i if (events is not None or mark) else None     # timed steps bracket their exchange with ev_x[i]
                return pipe.submit(q, seed=seed, events=events)[:3]
            dist_, idx_, nc_, k64 = indexer.query_tensors(q, k=k, hash_times=P, seed=seed, want_keys=world > 1, check=False, events=events)
            if world > 1:
                if events is not None:
                    ev_x[i][0].record()
                dist_, idx_, nc_ = gather_and_merge(k64, nc_, k)
                if events is not None:
                    ev_x[i][1].record()
            return dist_, idx_, nc_

        # graph slots (r06) run whole batches concurrently on the slots' own streams: two scan kernels may share the chip, so events around one
        # of them no longer time it alone -- and a batch with scan events is launched eagerly instead of replayed.  The timed pipelined region
        # then runs WITHOUT scan events and the kernel is timed in a short sequential region of its own below (same batches, same seeds).
        graph_slots = pipe is not None and getattr(pipe, "graph", False)
        for i in range(warmup):
            device_step(i % B)
        fence()
        t0 = time.perf_counter()
        for i in range(steps):
            device_step(i, events=None if graph_slots else ev[i], mark=True)
        if pipe is not None:
            pipe.synchronize()
        fence()
        elapsed_dev = max_over_ranks(time.perf_counter() - t0)
        last_status = pipe.last_slot.status if pipe is not None else indexer.last_status
        n_tasks, overflow = (int(v) for v in last_status.cpu())
        assert overflow == 0 and not (pipe is not None and pipe.overflowed()), "segment table overflow inside the timed region"
        if graph_slots:
            for i in range(steps):     # the scan kernel alone on the chip: sequential steps on one stream, no exchange
                indexer.query_tensors(qb[i % B], k=k, hash_times=P, seed=1000 + i, want_keys=world > 1, check=False, events=ev[i])
            fence()
        scan_avg_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))

        # N=1, L2: the same K sequential device-resident steps with the OPT-IN folded L2 form (NLSH_METRIC_L2_EPS_FOLDED: (q + eps) - c, two
        # vector operations per element instead of three, one rounding per element away from the reference's order; never the default,
        # never `value` or `roofline`) -- reported beside the shipped bit-exact form
        folded = None
        if world == 1 and pipe is None and metric == "l2" and args.l2_form == "exact":
            ev_f = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            for a, b in ev_f:
                a.record(); b.record()
            indexer.l2_form = "folded"
            try:
                for i in range(max(warmup, 1)):
                    device_step(i % B)
                fence()
                t0 = time.perf_counter()
                for i in range(steps):
                    device_step(i, events=ev_f[i])
                fence()
                el_f = time.perf_counter() - t0
                folded = {"scan_avg_ms": float(np.mean([a.elapsed_time(b) for a, b in ev_f])), "device_resident_ms_per_step": 1e3 * el_f / steps,
                          "device_resident_qps": Q * steps / el_f, "algo": int(indexer.last_algo)}
                d_f, i_f, _, _ = indexer.query_tensors(qb[0], k=k, hash_times=P, seed=5000)
            finally:
                indexer.l2_form = "exact"
            # how far apart the two forms are on this batch: id lists that differ at all, and the largest relative distance difference
            # (tests/test_gpu_fullsize.py holds every difference to a k-th-distance tie within 1e-4 and recall@10 to equality)
            d_e, i_e, _, _ = indexer.query_tensors(qb[0], k=k, hash_times=P, seed=5000)
            both = (i_e >= 0) & (i_f >= 0)
            folded["id_lists_differing"] = int((i_e != i_f).any(1).sum().item())
            folded["max_rel_distance_diff"] = float(((d_e - d_f).abs() / d_e.abs().clamp(min=1.0))[both].max().item()) if bool(both.any()) else 0.0

        # N=1: the same K device-resident steps through the three-stage pipeline as well (what a serving loop would run; the
        # sequential region above is the one whose scan kernel is timed alone on the chip for the roofline)
        piped_qps = None
        if world == 1 and pipe is None:
            from nlsh_amd.pipeline import QueryPipeline
            alt = QueryPipeline(indexer, qb[0], k=k, hash_times=P, depth=3)
            for i in range(warmup):
                alt.submit(qb[i % B], seed=1000 + i)
            alt.synchronize()
            fence()
            t0 = time.perf_counter()
            for i in range(steps):
                alt.submit(qb[i % B], seed=1000 + i)
            alt.synchronize()
            fence()
            piped_qps = Q * steps / (time.perf_counter() - t0)
            assert not alt.overflowed()
            del alt

        # candidates per launch of the timed device steps (untimed recomputation with the same batches and probe seeds)
        sum_c, uniq_rows = [], []
        tables = dict(indexer._max_tasks)          # task tables as the timed steps saw them
        bucket_rows = (indexer.offsets[1:] - indexer.offsets[:-1]).long() if indexer.n_buckets else None
        for i in range(steps):
            sum_c.append(int(indexer.query_tensors(qb[i % B], k=k, hash_times=P, seed=1000 + i)[2].long().sum().item()))
            # rows of the buckets the batch probes at all, each counted ONCE: what a schedule that shares a fetched row between the
            # queries probing its bucket has to read at least (the bucket-major schedules' algorithmic bytes)
            if bucket_rows is not None:
                kk, nn = indexer.hash_device(qb[i % B], hash_times=P, seed=1000 + i)
                pos = torch.searchsorted(indexer.uniq_keys, kk.clamp(min=int(indexer.uniq_keys[0]), max=int(indexer.uniq_keys[-1]))).clamp(max=indexer.n_buckets - 1)
                hit = (indexer.uniq_keys[pos] == kk) & (torch.arange(kk.shape[1], device=dev)[None, :] < nn[:, None])
                uniq_rows.append(int(bucket_rows[torch.unique(pos[hit])].sum().item()))
            # every timed step (not only the last, whose status word was read above) fitted its task table
            needed, tkey = int(indexer.last_status.cpu()[0]), indexer._last_tkey
            assert tkey not in tables or needed <= tables[tkey], f"step {i}: {needed} tasks > table {tables[tkey]} inside the timed region"
        sum_c_local = float(np.mean(sum_c))
        unique_bytes = 4.0 * d * float(np.mean(uniq_rows)) if uniq_rows else 0.0
        algo_bytes = 4.0 * d * sum_c_local
        flops_per_pair = 3.0 * d if metric == "l2" else 2.0 * d      # (q-c), +eps, fma per element | one fma
        algo_flops = flops_per_pair * sum_c_local
        t_scan = scan_avg_ms * 1e-3

        # encoder (MFMA) utilisation on this rank's corpus rows, and the device's measured HBM copy rate next to the spec peak
        enc, copy_gbps = None, None
        if world == 1:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            hashing.hash_device(shard, n=1)
            e0.record()
            for _ in range(5):
                hashing.hash_device(shard, n=1)
            e1.record()
            torch.cuda.synchronize()
            enc_ms = e0.elapsed_time(e1) / 5
            dims_ = [d] + list(hidden) + [H]
            flops = 2.0 * sum(a_ * b_ for a_, b_ in zip(dims_[:-1], dims_[1:])) * shard.shape[0]
            enc = {"kernel": "encode_hash_kernel (fp32 MFMA 32x32x2, fused bits + keys)", "rows": int(shard.shape[0]), "ms": enc_ms,
                   "tflops": flops / (enc_ms * 1e-3) / 1e12, "peak_tflops": MFMA_F32_PEAK_TFLOPS,
                   "mfma_util": flops / (enc_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS}
            src = torch.empty((1 << 28,), dtype=torch.float32, device=dev)      # 1 GiB read + 1 GiB written per copy
            dst = torch.empty_like(src)
            dst.copy_(src)
            e0.record()
            for _ in range(5):
                dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            copy_gbps = 2.0 * src.numel() * 4 * 5 / (e0.elapsed_time(e1) * 1e-3) / 1e9
            del src, dst

        # HBM traffic / VALU instruction counts per launch: PMC numbers cannot be collected from inside the process; they
        # come from the committed rocprofv3 --pmc passes (a profiling run of its own, same workload) when the
        # workload matches, and are labelled as such.
        traffic, valu_insts, clock_held, traffic_src, dram_bytes = (None,) * 5
        if world == 1:
            traffic, valu_insts, clock_held, traffic_src, dram_bytes = traffic_entry(
                f"{args.workload}:{args.data}:{args.l2_form}", (N, d, Q, H, P, int(indexer.last_algo), int(indexer.last_window)), "learned" in hash_desc)

    result = None
    if rank == 0:
        if gt_file is not None and gt_file.shape[1] >= k:
            gt = gt_file[:, :k]                  # the dataset's own `neighbors` (nlsh/trainers/base.py:42: ground_truth[:, :K])
        else:
            corpus_d = torch.from_numpy(corpus_h).to(dev)
            gt = brute_force_topk(qb[0], corpus_d, k, metric).cpu().numpy()
            del corpus_d
    # untimed: all lists on every rank (rank 0 computes the recall from them)
    # every rank takes part in the (collective) protocol call the recall is computed from; ONE fixed probe seed at every N,
    # so recall@10 and the candidate counts are the same numbers at 1, 2, 4 and 8 GPUs
    if sharded is not None:
        ids0, nc0 = sharded.query(qb[0], k=k, hash_times=P, seed=5000, own_slice=False)
    else:
        ids0, nc0 = indexer.query(qb[0], k=k, hash_times=P, seed=5000)
    if rank == 0:
        recall = float(np.mean(calculate_recall(list(gt), ids0)))
        mean_c = float(np.mean(nc0))
        value = Q * steps / elapsed
        algo = indexer.last_algo
        result = {
            "metric": "queries/sec + recall@10, SIFT1M 128-d 16-bit hash, 1/2/4/8 GPU" if args.workload == "sift1m" else
                      "queries/sec + recall@10 (GloVe-1.2M 100-d cosine 24-bit: BASELINE.json configs[2], not the headline)",
            "value": value, "unit": "queries/s", "n_gpus": world, "steps": steps, "warmup": warmup,
            "ms_per_step": 1e3 * elapsed / steps, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32", "data": "real" if args.dataset else "synthetic",
            "recall_at_10": recall,
            "value_protocol": "Indexer.query(batch, k, hash_times) -> Python lists of ALL Q queries on the calling rank, K synchronous calls "
                              "(nlsh/trainers/base.py:93-96), the facade's DEFAULT settings: what an unmodified Trainer.fit gets.  protocol_qps_opt_in (--full) is the same "
                              "region with Indexer.defer_result_release = Indexer.untracked_results = True (host-side opt-ins, INTEGRATION.md)" +
                              ("" if world == 1 else f"; sharded x{world}: every rank scans all queries over its shard, one all-gather + merge, every rank builds all Q "
                               "lists -- the call is host-bound (Python list construction, ~0.9 ms per 10^4 queries at N=1), so `value` is ~flat in N BY CONSTRUCTION; "
                               "the figure that scales is named by scaling_value_key (--full)"),
            # N>1 only: the exchange as the data backend itself saw it (ranks counted by an all-reduce of ones, devices by an all-gather of PCI ids)
            "collective": collective,
            "protocol_median_qps": Q / float(np.median(call_s)),
            "protocol_call_ms": [round(1e3 * c, 3) for c in call_s],
            # the five quantities the reference's validation logs (nlsh/trainers/base.py:87-90,105-108), same names
            "test_metrics": {"test/n_indexes": stats["n_indexes"], "test/std_index_rows": stats["std_index_rows"], "test/recall": recall,
                             "test/query_size": mean_c, "test/qps": Q * steps / elapsed},
            "config": {"workload": f"{wl['cfg']}, N={N} d={d} Q={Q} H={H} k={k} hash_times={P}, {B} query batches in rotation",
                       "hash": hash_desc, "l2_form": args.l2_form if metric == "l2" else None, "window_rows": int(indexer.last_window),
                       "shape": {"N": N, "d": d, "Q": Q, "H": H, "hash_times": P, "algo": int(algo), "window_rows": int(indexer.last_window)},
                       "traffic_key": f"{args.workload}:{args.data}:{args.l2_form}",
                       "parallelism": (f"corpus {args.shard} sharded x{world} ({indexer._candidate_vectors_gpu.shape[0]} rows on rank 0)"
                                       ) if world > 1 else "single GPU",
                       "n_buckets": stats["n_indexes"], "bucket_mean": stats["mean"], "bucket_median": stats["median"],
                       "bucket_max": stats["max"], "mean_candidates_per_query": mean_c, "index_build_s": build_s, "index_rebuild_s": rebuild_s},
        }
        if args.full:
            kernel = {0: "scan_kernel (query-major)", 1: "bscan2_kernel (bucket-major, 8 queries in registers)",
                      2: "bscan3_kernel (bucket-major, LDS-tiled)"}[algo] + " " + metric
            if algo == _capi.SCAN_QUERY_MAJOR:
                roof = {"bound": "hbm", "kernel": kernel, "achieved": algo_bytes / t_scan / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s"}
                roof["frac"] = roof["achieved"] / roof["peak"]
            else:
                # The bucket-major schedules fetch a corpus row once per query GROUP, so SURVEY 8(d)'s per-pair bytes (4 d sum C_q) are not what
                # they move (that rate is `algorithmic_GBps`, above the HBM peak on the headline).  Two roofs can bind them, both priced on
                # ALGORITHMIC quantities measured live: fp32 vector issue on the 3 d (L2) / 2 d (cosine) flops per (query, candidate) pair, and
                # HBM on the bytes of the DISTINCT candidate rows of the batch (each has to be read at least once).  `bound` is the one with
                # the one with the clearly larger fraction (HBM needs 1.5x the VALU fraction to be named: where the two are close -- the skewed
                # headline, 0.23 vs 0.25 -- the ablations of DESIGN.md appendix A show that arithmetic issue binds, the traffic is 0.7 GB per
                # launch); the balanced hashes with tiny buckets stream (nearly) the whole corpus once per batch and are HBM-side.
                valu_frac = algo_flops / t_scan / 1e12 / VALU_F32_PEAK_TFLOPS
                hbm_frac = unique_bytes / t_scan / 1e9 / HBM_PEAK_GBPS
                if 1.5 * valu_frac >= hbm_frac:
                    roof = {"bound": "valu", "kernel": kernel, "achieved": algo_flops / t_scan / 1e12, "peak": VALU_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": valu_frac}
                else:
                    roof = {"bound": "hbm", "kernel": kernel, "achieved": unique_bytes / t_scan / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": hbm_frac}
                roof.update({"valu_frac": valu_frac, "hbm_frac_of_distinct_candidate_rows": hbm_frac, "distinct_candidate_row_bytes_per_launch": unique_bytes,
                             "note": "bucket-major schedules share a fetched row between the queries of a group: bound = (pair flops / fp32 vector peak) unless (bytes of the "
                                     "batch's distinct candidate rows / HBM peak) is more than 1.5x that fraction; both algorithmic and measured live, both reported; the contract's "
                                     "'mfma' slot does not apply (the distance math is VALU by design, north_star keeps MFMA for the encoder)"})
            roof.update({"traffic": traffic, "traffic_source": traffic_src, "avg_launch_ms": scan_avg_ms,
                         "algorithmic_bytes_per_launch": algo_bytes, "algorithmic_GBps": algo_bytes / t_scan / 1e9,
                         "algorithmic_flops_per_launch": algo_flops, "sum_candidates_per_launch": sum_c_local, "tasks_per_launch": n_tasks})
            if traffic:
                roof["hbm_frac_of_measured_traffic"] = traffic / t_scan / 1e9 / HBM_PEAK_GBPS
            if dram_bytes is not None:     # where the bytes come from, as far as the hardware counters go (profiles/traffic_r06.json: `origin`)
                roof["traffic_origin"] = dram_bytes
            if valu_insts:
                roof["valu_wave_instructions_per_launch"] = valu_insts
                roof["valu_issue_frac"] = valu_insts * 2.0 / (1024 * t_scan * 2.4e9)
                if clock_held:   # the chip holds less than 2.4 GHz in this kernel: the same fraction at that clock
                    roof["clock_held_GHz"] = clock_held
                    roof["valu_issue_frac_at_clock_held"] = valu_insts * 2.0 / (1024 * t_scan * clock_held * 1e9)
            if copy_gbps is not None:
                roof["hbm_copy_measured_GBps"] = copy_gbps
            result.update({
                "protocol_qps_opt_in": Q * steps / elapsed_opt_in,
                # the field of THIS line a scaling study should read: device-resident steps (results left in HBM, incl. the all-gather + merge at N>1);
                # predicted ceiling from the one-GPU emulation of the per-rank pipelined local step (profiles/r06_shard_step_profile_pipelined.jsonl:
                # 0.302 / 0.169 / 0.106 / 0.076 ms at 1 / 2 / 4 / 8 bucket shards, host enqueue 0.02 ms per batch through graph slots):
                # encode + lookup, the task layout and the merge are replicated on every rank
                "scaling_value_key": "device_resident_qps",
                "scaling_ceiling_note": "per-rank pipelined local step emulated on one GPU (graph slots, profiles/r06_shard_step_profile_pipelined.jsonl): 0.302 / 0.169 / 0.106 / 0.076 ms = x1.8 / x2.85 / x4.0 at N = 2 / 4 / 8 before the all-gather (the ~70 us of encode + lookup, task layout and merge every rank repeats; host enqueue 0.02 ms per batch)",
                "own_slice_qps": None if elapsed_own is None else Q * steps / elapsed_own,
                "device_resident_qps": Q * steps / elapsed_dev, "device_resident_ms_per_step": 1e3 * elapsed_dev / steps,
                "device_resident_pipelined_qps": piped_qps,
                "roofline": roof,
            })
            if world > 1:
                result["config"]["parallelism"] += (f", all-gather of per-shard top-k + merge: "
                                                    f"{float(np.mean([a.elapsed_time(b) for a, b in ev_x])):.4f} ms/step")
            result["config"]["device_step_driver"] = (("graph slots: every batch one captured hipGraph on its slot's own stream (nlsh_amd/pipeline.py)"
                                                       if graph_slots else "three-stage pipeline over three HIP streams (nlsh_amd/pipeline.py)")
                                                      if pipe is not None else "sequential: every kernel of a step back to back on one stream")
            if folded is not None and folded["algo"] == _capi.SCAN_BUCKET_TILED:
                result["l2_folded_opt_in"] = {
                    "form": "sqrt(sum(((q + 1e-6) - c)^2)): Indexer(l2_form='folded') / NLSH_METRIC_L2_EPS_FOLDED; |d - d_exact| <= 1e-4 * max(1, d), not "
                            "bit-identical to the oracle, NOT what value / roofline above measure",
                    "avg_launch_ms": folded["scan_avg_ms"], "achieved": algo_flops / (folded["scan_avg_ms"] * 1e-3) / 1e12, "unit": "TFLOP/s",
                    "frac_of_valu_peak_on_the_same_algorithmic_flops": algo_flops / (folded["scan_avg_ms"] * 1e-3) / 1e12 / VALU_F32_PEAK_TFLOPS,
                    "device_resident_ms_per_step": folded["device_resident_ms_per_step"], "device_resident_qps": folded["device_resident_qps"],
                    "id_lists_differing_from_exact": folded["id_lists_differing"], "of_queries": Q, "max_rel_distance_diff_vs_exact": folded["max_rel_distance_diff"],
                    "full_line": "python bench.py --l2-form folded prints the complete line (value, roofline, recall) measured on this form"}
            if enc is not None:
                result["encoder"] = enc
            if world == 1 and not args.no_cpu_baseline:
                result["cpu_baseline"] = cpu_baseline(args, corpus_h, batches_h[0], Ws, bs, indexer, qb[0], metric)
            side_ok = (world == 1 and not args.no_side_workloads and args.workload == "sift1m" and args.data == "manifold" and not args.dataset
                       and not args.n and not args.dim and not args.hash_size and args.l2_form == "exact" and args.algo is None and args.window is None)
            if side_ok:
                # the other two workloads the round's numbers are quoted on, driver-run like the headline; `folded` is
                # `l2_folded_opt_in` above (the headline's own index with the 2-op L2 form)
                del indexer, shard
                torch.cuda.empty_cache()
                result["workloads"] = {tag: side_workload(tag, args, dev) for tag in ("glove", "clusters")}
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _cpu_allowance():
    """(CPUs this process may run on, cgroup cpu.max string): what the lease really gives, next to os.cpu_count()."""
    try:
        affinity = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        affinity = os.cpu_count() or 1
    cg = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            cg = open(path).read().strip()
            break
        except OSError:
            continue
    cores = affinity
    if cg:
        parts = cg.split()
        try:
            if len(parts) == 2 and parts[0] != "max":
                cores = max(1, min(cores, int(float(parts[0]) / float(parts[1]) + 0.5)))
            elif len(parts) == 1 and int(parts[0]) > 0:
                cores = max(1, min(cores, int(int(parts[0]) / 100000 + 0.5)))
        except ValueError:
            pass
    return affinity, cg, cores


def cpu_baseline(args, corpus_h, queries_h, Ws, bs, indexer, queries, metric):
    """CPU restatements of the reference's path on a bounded sample of the same workload: same queries, same
    multi-probe keys (identical candidate sets), same k.  Two restatements are timed and the faster one is `value`:
    * "port": oracle/ C restatement -- BLAS forward + AVX2/OpenMP scan (8 candidates per lane set, bit-identical to the
      scalar oracle), at every CPU the lease allows and at 1 thread;
    * "torch": oracle/torch_restatement.py -- the reference's per-query Python loop over torch-CPU ops
      (nlsh/indexer.py:56-96: index_select gather -> F.pairwise_distance -> topk), at all cores and at 1 thread."""
    from oracle import oracle, torch_restatement
    k, P = args.k, args.hash_times
    seed = 4242
    keys, nkeys = indexer.hash_device(queries, hash_times=P, seed=seed)
    kh, nh = keys.cpu().numpy().astype(np.int64), nkeys.cpu().numpy()
    ck = indexer.corpus_keys.cpu().numpy().astype(np.int64)
    mode = "ref_int16" if args.hash_size_eff <= 16 else "full"
    if mode == "full":  # full-width keys travel as int32 bit patterns
        ck, kh = ck & 0xFFFFFFFF, kh & 0xFFFFFFFF
    perm, uniq, offs = oracle.build_csr(ck)
    affinity, cgroup, cores = _cpu_allowance()
    Q = len(queries_h)

    def run_port(sample, simd=True):
        t0 = time.perf_counter()
        z = oracle.mlp_forward_blas(queries_h[:sample], Ws, bs)
        _, p01 = oracle.head_probs(z)
        oracle.row_keys(p01, P, mode, seed=seed, n_multi_rows=(sample // 4096) * 4096)
        t1 = time.perf_counter()
        oracle.query_batch(corpus_h, perm, uniq, offs, queries_h[:sample], kh[:sample], nh[:sample], k, metric, simd=simd)
        return t1 - t0, time.perf_counter() - t1

    def timed_port(threads, budget_s):
        oracle.set_num_threads(threads)
        probe = min(Q, 64 * max(1, threads // 8))
        th, ts = run_port(probe)
        per_q = (th + ts) / probe
        sample = int(min(Q, max(probe, budget_s / max(per_q, 1e-9))))
        passes, th, ts = 0, 0.0, 0.0
        while passes == 0 or (th + ts < budget_s and passes < 64):
            a, b = run_port(sample)
            th, ts, passes = th + a, ts + b, passes + 1
        return sample * passes / (th + ts), sample, passes, th, ts

    port_all = timed_port(cores, args.cpu_seconds)
    port_one = timed_port(1, min(args.cpu_seconds, 4.0))
    oracle.set_num_threads(cores)

    # the torch-CPU restatement: hashing through the torch module forward, scan through the per-query loop
    index2row = torch_restatement.build_index2row(perm, uniq, offs)
    corpus_t, queries_t = torch.from_numpy(corpus_h), torch.from_numpy(queries_h)
    module = indexer._hashing._hasher
    key_lists = [kh[i, :nh[i]].tolist() for i in range(Q)]

    def timed_torch(threads, budget_s):
        prev = torch.get_num_threads()
        torch.set_num_threads(threads)
        try:
            cpu_module = copy.deepcopy(module).cpu().eval()
            sample, total, done = 32, 0.0, 0
            while total < budget_s and done < Q:
                n = min(sample, Q - done)
                t0 = time.perf_counter()
                with torch.no_grad():
                    cpu_module(queries_t[done:done + n])                     # hashings.py:66-72 forward (+ sampling on the host)
                torch_restatement.query(corpus_t, index2row, queries_t[done:done + n], key_lists[done:done + n], k, metric)
                total += time.perf_counter() - t0
                done += n
                sample = min(sample * 2, 1024)
            return done / total, done
        finally:
            torch.set_num_threads(prev)

    torch_all = timed_torch(cores, min(args.cpu_seconds, 8.0))
    torch_one = timed_torch(1, min(args.cpu_seconds, 4.0))
    best_port = port_all[0] >= torch_all[0]
    out = {"value": port_all[0] if best_port else torch_all[0], "unit": "queries/s", "cores": cores,
           "kind": "port",
           "restatement": "oracle C (BLAS forward + AVX2/OpenMP scan)" if best_port else "torch-CPU per-query loop (oracle/torch_restatement.py)",
           "sample": (f"first {port_all[1]} of {Q} queries x {port_all[2]} passes, same keys/candidate sets as the GPU run; "
                      f"hash {port_all[3]:.3f}s (numpy BLAS) + scan {port_all[4]:.3f}s (C AVX2, OpenMP x{cores})"),
           "port_qps": {"threads": cores, "value": port_all[0], "one_thread": port_one[0], "thread_scaling": port_all[0] / port_one[0]},
           "torch_qps": {"threads": cores, "value": torch_all[0], "one_thread": torch_one[0], "queries_timed": torch_all[1],
                         "note": "reference algorithm restated with torch-CPU ops (python loop per query, as nlsh/indexer.py:56-96)"},
           "host_cpu_count": os.cpu_count(), "sched_affinity_cpus": affinity, "cgroup_cpu_max": cgroup, "host_cpu_model": _cpu_model()}
    return out


if __name__ == "__main__":
    main()
