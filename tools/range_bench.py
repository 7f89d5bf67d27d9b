#!/usr/bin/env python3
"""The batched RANGE (bloomhip_range_batch) on the C3 tree (workloads.c3_runs():
five level runs, 22.3M entries) with seeded values attached, runs, bounds and
outputs device-resident and warm.  Two legs:

  (a) 1M random ranges sized for about 100 results each (the wave class);
  (b) 16 ranges of 1/16 of the key domain each (the large class).

Per leg: the fill call and the count-only call, timed with device events
around the (synchronous) call and with the host clock, warm-up first, then
--repeats calls, median / min / max reported.  Compared with
  (a) the same answers computed on the host with numpy from host copies of
      the runs: searchsorted per run and query, the candidates gathered,
      sorted by (query, key, run), the first entry of every key kept;
  (b) bloomhip_compact called by hand on the same 16 x 5 sub-ranges.
The device answers are checked against the host's before anything is reported.

    python tools/range_bench.py [--out profiles/range_batch/range_bench.json]
    python tools/range_bench.py --prof 5 --leg a   # only range calls, for one
                                   # rocprofv3 --kernel-trace --stats run
"""
import argparse
import ctypes
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
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def setup():
    _, levels = W.c3_runs()
    runs, ents = [], []
    for lvl, keys, m in levels:
        f = bh.BloomFilter(m)
        f.set_batch_run(keys)
        rng = np.random.default_rng(VALUE_SEED + lvl)
        e = np.empty((keys.size, 2), dtype=np.int32)
        e[:, 0] = keys
        e[:, 1] = rng.integers(I32_MIN + 1, 2**31, size=keys.size, dtype=np.int64).astype(np.int32)
        runs.append(f)
        ents.append(e)
    return runs, ents


def host_ranges(ents, starts, ends):
    """The searchsorted-based host way: (offsets, entries)."""
    nq = starts.size
    qs, ks, vs, rs = [], [], [], []
    for r, e in enumerate(ents):
        k = e[:, 0]
        lo = np.searchsorted(k, starts, side="left")
        hi = np.maximum(np.searchsorted(k, ends, side="left"), lo)
        hi = np.where(ends <= starts, lo, hi)
        cnt = hi - lo
        q = np.repeat(np.arange(nq, dtype=np.int64), cnt)
        first = np.repeat(lo - (np.cumsum(cnt) - cnt), cnt)
        idx = first + np.arange(q.size, dtype=np.int64)
        qs.append(q)
        ks.append(k[idx])
        vs.append(e[idx, 1])
        rs.append(np.full(q.size, r, dtype=np.int8))
    q, k, v, r = (np.concatenate(x) for x in (qs, ks, vs, rs))
    # one sort by (query, key, run): 20 + 32 + 3 bits (nq <= 2^20, <= 8 runs)
    assert nq <= 1 << 20 and len(ents) <= 8
    order = np.argsort((q << 35) | ((k.astype(np.int64) + 2**31) << 3) | r)
    q, k, v = q[order], k[order], v[order]
    keep = np.ones(q.size, dtype=bool)
    keep[1:] = (q[1:] != q[:-1]) | (k[1:] != k[:-1])
    keep &= v != I32_MIN
    q, k, v = q[keep], k[keep], v[keep]
    offsets = np.zeros(nq + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.bincount(q, minlength=nq))
    return offsets, np.stack([k, v], axis=1)


def summary(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4),
            "max_ms": round(xs[-1], 4), "calls": len(xs)}


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return {"device_events": summary(ev), "host_clock": summary(wall)}


class Leg:
    def __init__(self, runs, dents, starts, ends):
        self.runs, self.dents = runs, dents
        self.nq = starts.size
        self.ds = torch.from_numpy(starts).cuda()
        self.de = torch.from_numpy(ends).cuda()
        self.offs = torch.empty(self.nq + 1, dtype=torch.int64, device="cuda")
        self.out = None
        nr = len(runs)
        self.h = (ctypes.c_void_p * nr)(*[r.handle.value for r in runs])
        self.e = (ctypes.c_void_p * nr)(*[d.data_ptr() for d in dents])
        self.n = (ctypes.c_size_t * nr)(*[d.shape[0] for d in dents])

    def count(self):
        total = ctypes.c_size_t()
        rc = bh.lib().bloomhip_range_batch(self.h, self.e, self.n, len(self.runs), 1, self.ds.data_ptr(),
                                           self.de.data_ptr(), self.nq, 1, self.offs.data_ptr(), None, 0,
                                           ctypes.byref(total), 1, 0, None)
        assert rc == bh.OK, rc
        return total.value

    def fill(self):
        if self.out is None:
            self.out = torch.empty((self.count(), 2), dtype=torch.int32, device="cuda")
        return bh.range_batch(self.runs, self.dents, self.ds, self.de, out=self.out, offsets=self.offs)

    def check(self, ents, starts, ends):
        t0 = time.perf_counter()
        want_off, want_out = host_ranges(ents, starts, ends)
        host_ms = (time.perf_counter() - t0) * 1e3
        off, out = self.fill()
        ok = (np.array_equal(off.cpu().numpy().view(np.uint64), want_off)
              and np.array_equal(out.cpu().numpy(), want_out))
        return ok, host_ms, int(want_off[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_batch", "range_bench.json"))
    ap.add_argument("--prof", type=int, default=0)
    ap.add_argument("--leg", choices=["a", "b", "ab"], default="ab")
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert bh.device_count() > 0, "range_bench needs a GPU"

    runs, ents = setup()
    dents = [torch.from_numpy(e).cuda() for e in ents]
    total_entries = sum(e.shape[0] for e in ents)
    rng = np.random.default_rng(99)
    width = int(round(100 * 2**32 / total_entries))
    sa = rng.integers(I32_MIN, I32_MAX - width, size=args.queries, dtype=np.int64)
    ea = sa + width
    sb = I32_MIN + np.arange(16, dtype=np.int64) * 2**28
    eb = np.minimum(sb + 2**28, I32_MAX)
    legs = {}
    if "a" in args.leg:
        legs["a"] = (Leg(runs, dents, sa.astype(np.int32), ea.astype(np.int32)), sa.astype(np.int32),
                     ea.astype(np.int32))
    if "b" in args.leg:
        legs["b"] = (Leg(runs, dents, sb.astype(np.int32), eb.astype(np.int32)), sb.astype(np.int32),
                     eb.astype(np.int32))

    if args.prof:
        for leg, _, _ in legs.values():
            leg.fill()
        torch.cuda.synchronize()
        for leg, _, _ in legs.values():
            for _ in range(args.prof):
                leg.fill()
            for _ in range(args.prof):
                leg.count()
        torch.cuda.synchronize()
        return

    res = {
        "tool": "tools/range_bench.py",
        "kernel_sha": bh.lib().bloomhip_kernel_sha().decode(),
        "device": torch.cuda.get_device_name(0),
        "workload": "c3_runs", "runs": len(runs),
        "run_entries": [int(e.shape[0]) for e in ents],
        "range_width_a": width, "repeats": args.repeats, "warmup": args.warmup,
    }
    for name, (leg, s, e) in legs.items():
        ok, host_ms, total = leg.check(ents, s, e)
        if not ok:
            print(json.dumps({"error": f"leg {name}: range_batch differs from the host's answers"}))
            sys.exit(1)
        r = {"queries": int(s.size), "results": total, "checked_against_host": True,
             "fill": timed(leg.fill, args.warmup, args.repeats),
             "count_only": timed(leg.count, args.warmup, args.repeats),
             "host_numpy_ms_single_run": round(host_ms, 1)}
        if name == "b":
            # the same 16 x 5 sub-ranges compacted by hand (bloomhip_compact)
            subs = []
            for q in range(s.size):
                row = []
                for d, h in zip(dents, ents):
                    lo, hi = np.searchsorted(h[:, 0], [s[q], e[q]])
                    row.append(d[lo:hi])
                subs.append(row)
            cout = torch.empty((max(sum(x.shape[0] for x in row) for row in subs), 2),
                               dtype=torch.int32, device="cuda")

            def by_hand():
                for row in subs:
                    bh.compact(row, drop_tombstones=True, out=cout)

            r["compact_by_hand_16_calls"] = timed(by_hand, args.warmup, args.repeats)
            r["candidates_per_query"] = [int(sum(x.shape[0] for x in row)) for row in subs]
        res["leg_" + name] = r
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
