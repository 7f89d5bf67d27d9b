#!/usr/bin/env python3
"""The batched PUT (bloomhip_flush_batch) with the new run's filter build fused
in, ops and output device-resident and warm.  Three shapes:

  (a) 16.8M ops, random keys: gen_puts(13141, 1 << 24, with_vals=True);
  (b) 16.8M ops on at most 4.2M distinct keys (keys of (a) drawn again);
  (c) 1000 ops (a b = 1000 memtable), through the one-workgroup path and
      through the tiled path (BLOOMHIP_FLUSH_PATH=tiled).

Two yardsticks, run in the same process on the same ops, in rounds interleaved
with the call, and checked equal to its output (run and filter words) first:

  (1) host: numpy stable argsort of the keys, the last op of every key kept,
      then set_batch_run of the run's keys (host clock);
  (2) torch on the device: stable torch.sort of the keys, a gather of the ops,
      a keep-last mask, then set_batch_run of the run (stride 8).

Device legs are timed with events around the (synchronous) call and with the
host clock; median / min / max over --repeats rounds after --warmup.

    python tools/flush_bench.py [--out profiles/flush_batch/flush_bench.json]
    python tools/flush_bench.py --prof 5 --shape a   # only flush calls, for one
                                   # rocprofv3 --kernel-trace --stats run
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

BPE = 10.0


def shapes(which):
    keys, vals = bh.gen_puts(13141, 1 << 24, with_vals=True)
    out = {}
    if "a" in which:
        out["a"] = np.stack([keys, vals], axis=1)
    if "b" in which:
        rng = np.random.default_rng(4242)
        out["b"] = np.stack([keys[rng.integers(0, 1 << 22, size=keys.size)], vals], axis=1)
    if "c" in which:
        out["c"] = np.stack([keys[:1000], vals[:1000]], axis=1)
    return {k: np.ascontiguousarray(v.astype(np.int32)) for k, v in out.items()}


def summary(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4),
            "max_ms": round(xs[-1], 4), "calls": len(xs)}


class Shape:
    def __init__(self, ops):
        self.ops = ops
        self.n = ops.shape[0]
        self.d_ops = torch.from_numpy(ops).cuda()
        self.d_out = torch.empty((self.n, 2), dtype=torch.int32, device="cuda")
        m = bh.m_bits(self.n, BPE)
        self.f_call, self.f_torch, self.f_host = (bh.BloomFilter(m) for _ in range(3))

    def call(self, path="auto"):
        os.environ["BLOOMHIP_FLUSH_PATH"] = path
        self.f_call.clear()
        return bh.flush_batch(self.d_ops, filter=self.f_call, out=self.d_out)

    def torch_way(self):
        sk, idx = torch.sort(self.d_ops[:, 0], stable=True)
        keep = torch.ones(self.n, dtype=torch.bool, device="cuda")
        keep[:-1] = sk[1:] != sk[:-1]  # the last op of every key
        run = self.d_ops[idx[keep]]
        self.f_torch.clear()
        self.f_torch.set_batch_run(run, stride=8)
        torch.cuda.synchronize()
        return run

    def host_way(self):
        k = self.ops[:, 0]
        order = np.argsort(k, kind="stable")
        sk = k[order]
        keep = np.ones(self.n, dtype=bool)
        keep[:-1] = sk[1:] != sk[:-1]
        run = self.ops[order[keep]]
        self.f_host.clear()
        self.f_host.set_batch_run(np.ascontiguousarray(run[:, 0]))
        return run

    def check(self, paths):
        want = self.host_way()
        ok = np.array_equal(self.torch_way().cpu().numpy(), want)
        ok = ok and np.array_equal(self.f_torch.words(), self.f_host.words())
        for p in paths:
            self.f_call.clear()
            ok = ok and np.array_equal(self.call(p).cpu().numpy(), want)
            ok = ok and np.array_equal(self.f_call.words(), self.f_host.words())
            ok = ok and np.array_equal(self.f_call.run_meta()[0], self.f_host.run_meta()[0])
        return ok, int(want.shape[0])


def time_device(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flush_batch", "flush_bench.json"))
    ap.add_argument("--prof", type=int, default=0)
    ap.add_argument("--shape", default="abc")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-repeats", type=int, default=2)
    args = ap.parse_args()
    assert bh.device_count() > 0, "flush_bench needs a GPU"
    todo = {name: Shape(ops) for name, ops in shapes(args.shape).items()}

    if args.prof:
        for name, s in todo.items():
            for p in (("auto", "tiled") if name == "c" else ("auto",)):
                for _ in range(args.prof + 1):
                    s.call(p)
        torch.cuda.synchronize()
        return

    res = {"tool": "tools/flush_bench.py", "kernel_sha": bh.lib().bloomhip_kernel_sha().decode(),
           "device": torch.cuda.get_device_name(0), "bits_per_entry": BPE,
           "repeats": args.repeats, "warmup": args.warmup,
           "flush_tile": bh.FLUSH_TILE, "flush_block_cap": bh.FLUSH_BLOCK_CAP}
    for name, s in todo.items():
        paths = ("auto", "tiled") if name == "c" else ("auto",)
        ok, distinct = s.check(paths)
        if not ok:
            print(json.dumps({"error": f"shape {name}: flush_batch differs from a yardstick"}))
            sys.exit(1)
        legs = {("flush_batch_" + p): (lambda p=p: s.call(p)) for p in paths}
        legs["torch_sort_pipeline"] = s.torch_way
        times = {k: ([], []) for k in legs}
        for r in range(args.warmup + args.repeats):  # interleaved rounds
            for k, fn in legs.items():
                ev, wall = time_device(fn)
                if r >= args.warmup:
                    times[k][0].append(ev)
                    times[k][1].append(wall)
        host = []
        for _ in range(args.host_repeats):
            t0 = time.perf_counter()
            s.host_way()
            host.append((time.perf_counter() - t0) * 1e3)
        r = {"ops": s.n, "distinct_keys": distinct, "checked_against_both_yardsticks": True}
        for k, (ev, wall) in times.items():
            r[k] = {"device_events": summary(ev), "host_clock": summary(wall)}
        r["host_numpy_pipeline"] = {"host_clock": summary(host)}
        res["shape_" + name] = r
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
