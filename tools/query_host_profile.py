#!/usr/bin/env python3
"""Where one `Indexer.query()` call of the headline workload spends its wall time (host stamps around its stages)."""
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nlsh_amd import io, synth  # noqa: E402
from nlsh_amd.data import SIFT  # noqa: E402
from nlsh_amd.indexer import Indexer  # noqa: E402

N, d, Q = 1_000_000, 128, 10_000
corpus_h, mean, std = synth.standardise(synth.sift_manifold(N, d, seed=synth.SEED_DATA))
queries_h, _, _ = synth.standardise(synth.sift_manifold(Q, d, seed=synth.SEED_QUERY), mean, std)
Ws, bs = io.load_hasher_weights(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "checkpoints", "sift1m_manifold_h16.npz"))
ix = Indexer(io.hashing_from_weights(Ws, bs, compat=True), torch.from_numpy(corpus_h).cuda(), SIFT.distance)
q = torch.from_numpy(queries_h).cuda()
for _ in range(5):
    ix.query(q, 10, 10)
T = {k: [] for k in ("hash_launch", "scan_launch+copies", "sync_wait", "tolist", "f7+rest", "total")}
now = time.perf_counter
sync = torch.cuda.current_stream().synchronize
for _ in range(30):
    torch.cuda.synchronize()
    t0 = now()
    keys, nkeys = ix.hash_device(q, hash_times=10)
    t1 = now()
    orig = torch.cuda.Stream.synchronize
    stamps = []
    def timed(self_, _o=orig):
        stamps.append(now()); _o(self_); stamps.append(now())
    torch.cuda.Stream.synchronize = timed
    try:
        idx_h, nc_h, keys_h, nkeys_h = ix._host_results(q, keys, nkeys, 10)
    finally:
        torch.cuda.Stream.synchronize = orig
    t3 = now()
    res, counts = ix._plain_lists(idx_h, nc_h)
    t4 = now()
    short = np.nonzero(nc_h < 10)[0]
    t5 = now()
    T["hash_launch"].append(t1 - t0); T["scan_launch+copies"].append(stamps[0] - t1); T["sync_wait"].append(stamps[1] - stamps[0])
    T["tolist"].append(t4 - t3); T["f7+rest"].append(t5 - t4 + (t3 - stamps[1])); T["total"].append(t5 - t0)
whole = []
for _ in range(30):
    torch.cuda.synchronize(); t0 = now(); ix.query(q, 10, 10); whole.append(now() - t0)
print(json.dumps({k: round(1e3 * float(np.median(v)), 4) for k, v in T.items()} | {"query_call_median_ms": round(1e3 * float(np.median(whole)), 4), "short_queries": int(len(short))}))
if os.environ.get("QCHUNKS"):
    for ch in [int(v) for v in os.environ["QCHUNKS"].split(",")]:
        ix.query_chunks = ch
        for _ in range(5):
            ix.query(q, 10, 10)
        w, keep = [], None
        for _ in range(60):
            torch.cuda.synchronize(); t0 = now(); keep = ix.query(q, 10, 10); t1 = now(); w.append(t1 - t0)
        loop0 = now()
        for _ in range(60):
            keep = ix.query(q, 10, 10)
        loop = (now() - loop0) / 60
        print(json.dumps({"query_chunks": ch, "call_median_ms": round(1e3 * float(np.median(w)), 4), "call_mean_ms": round(1e3 * float(np.mean(w)), 4),
                          "loop_ms_per_call_incl_free_of_previous": round(1e3 * loop, 4)}))
    # the same calls with stamps inside them: where the host is while the ranges run.  "shells" = the containers built between the last
    # launch and the first wait (csrc/fastlists.c rows_alloc), "wait" = what is left of the idle time (event / stream synchronise),
    # "fill" = the ids and counts stored per range (rows_fill; one-shot: rows_to_lists), "before_wait" = hashing call, launches and the
    # release of nothing (the result is kept here), "rest" = short-query rule, key sets, Python between the stages.  Both constructions
    # in one process: "one_shot" is the path with the two-phase helper taken away (the parent commit's).
    from nlsh_amd import indexer as ixmod
    helper = ixmod._rows_alloc, ixmod._rows_fill, ixmod._rows_to_lists
    ev_sync, st_sync = torch.cuda.Event.synchronize, torch.cuda.Stream.synchronize
    for ch in [int(v) for v in os.environ["QCHUNKS"].split(",")]:
        for mode in ("one_shot", "two_phase"):
            if mode == "two_phase" and helper[0] is None:
                continue
            ix.query_chunks = ch
            acc, first_wait = {}, []

            def stamped(fn, key):
                def inner(*a, **kw):
                    t = now()
                    if key == "wait" and not first_wait:
                        first_wait.append(t)
                    try:
                        return fn(*a, **kw)
                    finally:
                        acc[key] = acc.get(key, 0.0) + now() - t
                return inner
            ixmod._rows_alloc, ixmod._rows_fill = (stamped(helper[0], "shells"), stamped(helper[1], "fill")) if mode == "two_phase" else (None, None)
            ixmod._rows_to_lists = stamped(helper[2], "fill") if helper[2] is not None else None
            torch.cuda.Event.synchronize, torch.cuda.Stream.synchronize = stamped(ev_sync, "wait"), stamped(st_sync, "wait")
            S = {k_: [] for k_ in ("before_wait", "shells", "wait", "fill", "rest", "total")}
            try:
                for it in range(45):
                    acc.clear(); del first_wait[:]
                    st_sync(torch.cuda.current_stream())
                    t0 = now(); keep = ix.query(q, 10, 10); t1 = now()
                    if it < 5:
                        continue
                    shells = acc.get("shells", 0.0)
                    S["before_wait"].append(first_wait[0] - t0 - shells); S["shells"].append(shells); S["wait"].append(acc.get("wait", 0.0))
                    S["fill"].append(acc.get("fill", 0.0)); S["total"].append(t1 - t0)
                    S["rest"].append(t1 - t0 - (first_wait[0] - t0) - acc.get("wait", 0.0) - acc.get("fill", 0.0))
            finally:
                ixmod._rows_alloc, ixmod._rows_fill, ixmod._rows_to_lists = helper
                torch.cuda.Event.synchronize, torch.cuda.Stream.synchronize = ev_sync, st_sync
            print(json.dumps({"query_chunks": ch, "construction": mode} | {k_: round(1e3 * float(np.median(v_)), 4) for k_, v_ in S.items()}))
    ix.query_chunks = None
if os.environ.get("QINLINE"):
    from nlsh_amd.hashings import host_key_set
    S = {k: [] for k in ("as_queries", "hash_device", "host_results", "f7_keysets", "plain_lists", "f7_rows", "dealloc_prev", "total")}
    prev = None
    for _ in range(40):
        torch.cuda.synchronize()
        t0 = now(); qq = ix._as_queries(q)
        t1 = now(); keys, nkeys = ix.hash_device(qq, hash_times=10)
        t2 = now(); idx_h, nc_h, keys_h, nkeys_h = ix._host_results(qq, keys, nkeys, 10)
        t3 = now()
        key_sets = {}
        for qi in np.nonzero(nc_h < 10)[0].tolist():
            key_sets[qi] = host_key_set(keys_h[qi], int(nkeys_h[qi]), ix._hashing.key_mode)
        t4 = now(); results, counts = ix._plain_lists(idx_h, nc_h)
        t5 = now()
        for qi in np.nonzero(nc_h < 10)[0].tolist():
            order = list(key_sets[qi])
            results[qi] = ix._rows_of_key(order[-1]) if order else []
        t6 = now(); prev = (results, counts); results = counts = None
        t7 = now()
        for k_, v_ in zip(S, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t6 - t5, t7 - t6, t7 - t0)):
            S[k_].append(v_)
    print(json.dumps({k_: round(1e3 * float(np.median(v_)), 4) for k_, v_ in S.items()}))
if os.environ.get("QGC"):
    log = []
    def cb(phase, info, _t=[0.0]):
        if phase == "start":
            _t[0] = now()
        else:
            log.append((info["generation"], info["collected"], round(1e3 * (now() - _t[0]), 4)))
    gc.callbacks.append(cb)
    for _ in range(5):
        del log[:]
        t0 = now(); r = ix.query(q, 10, 10); t1 = now()
        print("query %.3f ms; collections (gen, collected, ms):" % (1e3 * (t1 - t0)), log, "gc counts", gc.get_count(), "thresholds", gc.get_threshold())
    gc.callbacks.remove(cb)
if os.environ.get("QPROFILE"):
    import cProfile
    import pstats
    pr = cProfile.Profile()
    pr.enable()
    for _ in range(30):
        r = ix.query(q, 10, 10)
    pr.disable()
    pstats.Stats(pr).sort_stats("tottime").print_stats(18)
