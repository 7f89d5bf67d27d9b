#!/usr/bin/env python3
"""Batched ingest into the tree handle (LSMTree.put_batch) against the cascade
the engine's user had to drive by hand before it, on 16.8M device-resident ops
(gen_puts(13141, 1 << 24, with_vals=True)), warm, in one process.  Two shapes:

  (a) B = 512,000, depth 5, fanout 10, 0.5 bits per entry (the reference's
      defaults, src/lsm_tree.h:9-13);
  (b) B = 512, the reference's `-b 1` tree.

Legs, in interleaved rounds (--repeats after --warmup), device events around
the synchronous calls and the host clock:

  (1) tree_put_batch   LSMTree.put_batch of the whole stream into an empty tree;
  (2) cascade_by_hand  one flush_batch per segment and one compact per
      merge_down, in the reference's order (src/lsm_tree.cpp:44-139), the cut
      points given (they are not timed here: a host loop over the ops finds
      them in tens of seconds).  At shape (b) the cascade is timed on the
      first --prefix ops and scaled by ops / prefix; the JSON says so;
  (3) flush_cuts       the cut points alone.

Before timing, the tree's runs are checked equal to the cascade's, and the cuts
equal to a host loop's on the first 200,000 ops.

    python tools/tree_bench.py [--out profiles/tree_ingest/tree_bench.json]
    python tools/tree_bench.py --prof 3 --shape a   # only put_batch calls, for
                                   # one rocprofv3 --kernel-trace --stats run
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

SHAPES = {"a": dict(B=512_000, depth=5, fanout=10, bpe=0.5),
          "b": dict(B=512, depth=5, fanout=10, bpe=0.5)}


def summary(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4),
            "max_ms": round(xs[-1], 4), "calls": len(xs)}


def time_device(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def host_cuts(keys, B):
    cuts, buf = [], set()
    for i, k in enumerate(keys.tolist()):
        if len(buf) >= B:
            cuts.append(i)
            buf = set()
        buf.add(k)
    return cuts


class Cascade:
    """The reference's flushes and merge_downs, one engine call each."""

    def __init__(self, d_ops, cuts, B, depth, fanout, bpe):
        self.d_ops, self.cuts = d_ops, [0] + [int(c) for c in cuts]
        self.depth, self.fanout = depth, fanout
        self.m = [bh.m_bits(B * fanout ** l, bpe) for l in range(depth)]
        self.levels = [[] for _ in range(depth)]  # newest first: (entries tensor, filter)
        self.calls = 0

    def merge_down(self, l):
        if len(self.levels[l]) < self.fanout:
            return
        assert l + 1 < self.depth, "No more space in tree"
        if len(self.levels[l + 1]) >= self.fanout:
            self.merge_down(l + 1)
        runs = [r[0] for r in self.levels[l]]
        out = torch.empty((sum(r.shape[0] for r in runs), 2), dtype=torch.int32, device="cuda")
        f = bh.BloomFilter(self.m[l + 1])
        merged = bh.compact(runs, drop_tombstones=l + 1 == self.depth - 1, filter=f, out=out)
        self.levels[l] = []
        self.levels[l + 1].insert(0, (merged, f))
        self.calls += 1

    def run(self):
        for a, b in zip(self.cuts[:-1], self.cuts[1:]):
            self.merge_down(0)
            out = torch.empty((b - a, 2), dtype=torch.int32, device="cuda")
            f = bh.BloomFilter(self.m[0])
            self.levels[0].insert(0, (bh.flush_batch(self.d_ops[a:b], filter=f, out=out), f))
            self.calls += 1
        return self


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_ingest", "tree_bench.json"))
    ap.add_argument("--prof", type=int, default=0)
    ap.add_argument("--shape", default="ab")
    ap.add_argument("--ops", type=int, default=1 << 24)
    ap.add_argument("--prefix", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert bh.device_count() > 0, "tree_bench needs a GPU"
    keys, vals = bh.gen_puts(13141, args.ops, with_vals=True)
    ops = np.ascontiguousarray(np.stack([keys, vals], axis=1).astype(np.int32))
    d_ops = torch.from_numpy(ops).cuda()

    def put_batch(cfg):
        t = bh.LSMTree(cfg["B"], cfg["depth"], cfg["fanout"], cfg["bpe"])
        return t, t.put_batch(d_ops)

    if args.prof:
        for name in args.shape:
            for _ in range(args.prof + 1):
                put_batch(SHAPES[name])[0].close()
        torch.cuda.synchronize()
        return

    res = {"tool": "tools/tree_bench.py", "kernel_sha": bh.lib().bloomhip_kernel_sha().decode(),
           "device": torch.cuda.get_device_name(0), "ops": args.ops, "repeats": args.repeats,
           "warmup": args.warmup, "tree_cut_chunk": bh.TREE_CUT_CHUNK}
    for name in args.shape:
        cfg = SHAPES[name]
        B = cfg["B"]
        cuts = bh.flush_cuts(d_ops, B)
        nhost = min(200_000, args.ops)
        ok = [int(c) for c in cuts if c < nhost] == host_cuts(ops[:nhost, 0], B)
        # the cascade of the whole stream (a) or of the prefix (b), against the tree
        part = args.ops if name == "a" else min(args.prefix, args.ops)
        part_cuts = [int(c) for c in cuts if c <= part]
        tree = bh.LSMTree(B, cfg["depth"], cfg["fanout"], cfg["bpe"])
        nfl = tree.put_batch(d_ops[:part_cuts[-1] + 1] if name == "b" else d_ops)
        casc = Cascade(d_ops, part_cuts, B, cfg["depth"], cfg["fanout"], cfg["bpe"]).run()
        ok = ok and nfl == len(part_cuts) and tree.shape()[0] == [len(lv) for lv in casc.levels]
        for l, lv in enumerate(casc.levels):
            for i, (ents, f) in enumerate(lv):
                got, view = tree.run(l, i)
                ok = ok and np.array_equal(got, ents.cpu().numpy())
                ok = ok and np.array_equal(view.words(), f.words())
        tree.close()
        if not ok:
            print(json.dumps({"error": f"shape {name}: the tree differs from the cascade"}))
            sys.exit(1)
        calls = casc.calls
        del casc

        def leg_tree():
            put_batch(cfg)[0].close()

        def leg_cascade():
            Cascade(d_ops, part_cuts, B, cfg["depth"], cfg["fanout"], cfg["bpe"]).run()

        legs = {"tree_put_batch": leg_tree, "cascade_by_hand": leg_cascade,
                "flush_cuts": lambda: bh.flush_cuts(d_ops, B)}
        times = {k: ([], []) for k in legs}
        for r in range(args.warmup + args.repeats):
            for k, fn in legs.items():
                ev, wall = time_device(fn)
                if r >= args.warmup:
                    times[k][0].append(ev)
                    times[k][1].append(wall)
        r = {**cfg, "flushes": int(cuts.size), "checked_against_the_cascade": True,
             "cascade_ops": part_cuts[-1], "cascade_engine_calls": calls,
             "cascade_scale_to_whole_stream": round(args.ops / part_cuts[-1], 3)}
        for k, (ev, wall) in times.items():
            r[k] = {"device_events": summary(ev), "host_clock": summary(wall)}
        r["cascade_by_hand"]["scaled_median_ms"] = round(
            r["cascade_by_hand"]["host_clock"]["median_ms"] * args.ops / part_cuts[-1], 2)
        res["shape_" + name] = r
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
