#!/usr/bin/env python3
"""The batched GET at the C3 routing workload (workloads.c3_runs(): five level
runs, 16.8M GETs) with seeded values attached, everything device-resident and
warm:

  (a) route_gets_packed alone,
  (b) get_batch, with the binary and the interpolated interval search,
  (c) the way without get_batch: routing on the GPU, the candidate rows
      copied to the host, resolution in numpy against host copies of the runs.

(b)'s vals, found_run and stats are checked against (c)'s before anything is
reported.  (a) and (b) are timed with device events in windows of about 0.2 s,
the variants alternating, five windows each; (c) with the host clock.

    python tools/get_bench.py [--out profiles/get_batch/get_bench.json]
    python tools/get_bench.py --prof 20     # only get_batch calls, for
                                            # rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs265-lsm-tree_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bloomhip as bh  # noqa: E402
from bloomhip import workloads as W  # noqa: E402

VALUE_SEED = 4242


def setup():
    gets, levels = W.c3_runs()
    runs, ents = [], []
    for lvl, keys, m in levels:
        f = bh.BloomFilter(m)
        f.set_batch_run(keys)
        rng = np.random.default_rng(VALUE_SEED + lvl)
        e = np.empty((keys.size, 2), dtype=np.int32)
        e[:, 0] = keys
        e[:, 1] = rng.integers(-2**31 + 1, 2**31, size=keys.size, dtype=np.int64).astype(np.int32)
        runs.append(f)
        ents.append(e)
    return gets, runs, ents


def host_resolve(cand, ents, gets):
    """Resolution of routed GETs on the host: per run, newest first, the
    still unanswered candidates are looked up in the run's sorted keys."""
    n = gets.size
    found = np.full(n, -1, dtype=np.int32)
    vals = np.full(n, bh.VAL_NONE, dtype=np.int32)
    stats = np.zeros((len(ents), 2), dtype=np.uint64)
    for r, e in enumerate(ents):
        c = np.unpackbits(cand[r].view(np.uint8), bitorder="little")[:n].astype(bool)
        idx = np.flatnonzero(c & (found < 0))
        k = gets[idx]
        pos = np.minimum(np.searchsorted(e[:, 0], k), e.shape[0] - 1)
        hit = e[pos, 0] == k
        found[idx[hit]] = r
        vals[idx[hit]] = e[pos[hit], 1]
        stats[r] = (idx.size, idx.size - int(hit.sum()))
    return vals, found, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "get_batch", "get_bench.json"))
    ap.add_argument("--prof", type=int, default=0)
    ap.add_argument("--window-s", type=float, default=0.2)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    assert bh.device_count() > 0, "get_bench needs a GPU"

    gets, runs, ents = setup()
    n, nr = gets.size, len(runs)
    nw = (n + 63) // 64
    dk = torch.from_numpy(gets).cuda()
    dents = [torch.from_numpy(e).cuda() for e in ents]
    dc = torch.zeros((nr, nw), dtype=torch.int64, device="cuda")
    dr = torch.empty(n, dtype=torch.int32, device="cuda")
    dv = torch.empty(n, dtype=torch.int32, device="cuda")
    df = torch.empty(n, dtype=torch.int32, device="cuda")
    ds = torch.zeros((nr, 2), dtype=torch.int64, device="cuda")

    def route():
        bh.route_gets_packed(runs, dk, cand=dc, route=dr)

    def get(search):
        os.environ["BLOOMHIP_GET_SEARCH"] = search
        bh.get_batch(runs, dents, dk, vals=dv, found_run=df, stats=ds)

    if args.prof:
        for search in ("binary", "interp"):
            get(search)
        torch.cuda.synchronize()
        for _ in range(args.prof):
            get("binary")
        for _ in range(args.prof):
            get("interp")
        torch.cuda.synchronize()
        return

    # (c), which is also the reference for (b)
    host_ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        cand, _ = bh.route_gets_packed(runs, dk, cand=np.zeros((nr, nw), dtype=np.uint64))
        t1 = time.perf_counter()
        want = host_resolve(cand, ents, gets)
        host_ms.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
    checks = {}
    for search in ("binary", "interp"):
        ds.fill_(-1)
        get(search)
        torch.cuda.synchronize()
        ok = (np.array_equal(dv.cpu().numpy(), want[0]) and np.array_equal(df.cpu().numpy(), want[1])
              and np.array_equal(ds.cpu().numpy().view(np.uint64), want[2]))
        checks[search] = bool(ok)
    if not all(checks.values()):
        print(json.dumps({"error": "get_batch differs from the host resolution", "checks": checks}))
        sys.exit(1)

    variants = {"route_gets_packed": route, "get_batch_binary": lambda: get("binary"),
                "get_batch_interp": lambda: get("interp")}
    per_call = {}
    for name, fn in variants.items():  # warm, and size the windows
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(3):
            fn()
        b.record()
        torch.cuda.synchronize()
        per_call[name] = a.elapsed_time(b) / 3
    samples = {name: [] for name in variants}
    for _ in range(args.windows):
        for name, fn in variants.items():
            k = max(3, int(args.window_s * 1e3 / per_call[name]))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(k):
                fn()
            b.record()
            torch.cuda.synchronize()
            samples[name].append(a.elapsed_time(b) / k)

    def summary(xs):
        xs = sorted(xs)
        return {"median_ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4),
                "max_ms": round(xs[-1], 4), "windows": len(xs)}

    # the resolve kernel alone, bracketed by the library's own events
    kernel_ms = {}
    for search in ("binary", "interp"):
        runs[0].profile(True)
        runs[0].profile_reset()
        for _ in range(20):
            get(search)
        prof = runs[0].profile_read()
        runs[0].profile(False)
        kernel_ms[search] = {k: round(v["ms"] / v["launches"], 4) for k, v in prof.items()}

    stats = want[2]
    reads = int(stats[:, 0].sum())
    res = {
        "tool": "tools/get_bench.py",
        "kernel_sha": bh.lib().bloomhip_kernel_sha().decode(),
        "device": torch.cuda.get_device_name(0),
        "workload": "c3_runs", "gets": int(n), "runs": nr,
        "run_entries": [int(e.shape[0]) for e in ents],
        "checks_against_host_resolution": checks,
        "route_gets_packed": summary(samples["route_gets_packed"]),
        "get_batch_binary": summary(samples["get_batch_binary"]),
        "get_batch_interp": summary(samples["get_batch_interp"]),
        "host_way_ms": {"total": [round(t, 1) for t, _ in host_ms],
                        "route_and_copy": [round(t, 1) for _, t in host_ms]},
        "per_slot_ms": kernel_ms,
        "answered": int((want[1] >= 0).sum()),
        "page_reads_per_run": stats[:, 0].tolist(),
        "false_reads_per_run": stats[:, 1].tolist(),
        "false_positive_rate_per_run": [round(float(f) / float(r), 5) if r else None
                                        for r, f in stats.tolist()],
        "resolve_bytes_streamed": int(4 * n + 8 * nr * nw + 8 * n),
        "resolve_search_bytes_max": reads * 13 * 64,
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
