"""A plain Python model of the reference's tree (jackdent/cs265-lsm-tree
src/lsm_tree.cpp:28-139, src/buffer.cpp:37-58), shared by the tree tests: a
dict buffer, lists of dict runs (newest first), merge_down as the reference
writes it.  The flush keeps tombstones; a merge into the last level drops them.
"""
TOMB = -2**31  # VAL_TOMBSTONE, src/types.h:12


class NoMoreSpace(Exception):
    """The reference dies with "No more space in tree" (src/lsm_tree.cpp:59)."""


class ModelTree:
    def __init__(self, B, depth, fanout):
        self.B, self.depth, self.fanout = B, depth, fanout
        self.buf = {}
        self.levels = [[] for _ in range(depth)]  # [level][newest first] -> {key: val}
        self.nops = 0
        self.cuts = []  # op index before which each flush happened

    def merge_down(self, l):
        if len(self.levels[l]) < self.fanout:
            return
        if l == self.depth - 1:
            raise NoMoreSpace()
        if len(self.levels[l + 1]) >= self.fanout:
            self.merge_down(l + 1)
        merged = {}
        for run in reversed(self.levels[l]):  # oldest first: newer values replace
            merged.update(run)
        if l + 1 == self.depth - 1:
            merged = {k: v for k, v in merged.items() if v != TOMB}
        self.levels[l] = []
        self.levels[l + 1].insert(0, merged)

    def put(self, key, val):
        if len(self.buf) >= self.B:  # Buffer::put refuses, even a key it holds
            self.merge_down(0)
            self.levels[0].insert(0, dict(self.buf))
            self.buf = {}
            self.cuts.append(self.nops)
        self.buf[key] = val
        self.nops += 1

    def delete(self, key):
        self.put(key, TOMB)

    def runs(self):
        """The buffer, then the runs in LSMTree::get_run order."""
        return [self.buf] + [r for lv in self.levels for r in lv]

    def get(self, key):
        """(value, run number): (TOMB, -1) when no run holds the key."""
        for i, run in enumerate(self.runs()):
            if key in run:
                return run[key], i
        return TOMB, -1

    def range(self, start, end):
        seen = {}
        for run in reversed(self.runs()):
            seen.update(run)
        return sorted((k, v) for k, v in seen.items() if start <= k < end and v != TOMB)

    def shape(self):
        return [len(lv) for lv in self.levels], len(self.buf)


def stream_cuts(keys, B):
    """The realised cuts of a key stream for a buffer of B entries."""
    t = ModelTree(B, 1, len(keys) + 2)
    for k in keys:
        t.put(int(k), 0)
    return t.cuts


def replay(test, tree_factory=None):
    """A recorded reference test (tests/golden/ref_tests.json) through the
    model: its stdout as the reference prints it (src/lsm_tree.cpp:173-290)."""
    B, depth, fanout = 512 * 1000, 5, 10  # src/lsm_tree.h:9-13
    p = test["params"]
    for flag, val in zip(p[::2], p[1::2]):
        if flag == "-b":
            B = 512 * int(val)
        elif flag == "-d":
            depth = int(val)
        elif flag == "-f":
            fanout = int(val)
    t = ModelTree(B, depth, fanout)
    out = []
    for op in test["ops"]:
        if op[0] == "p":
            t.put(op[1], op[2])
        elif op[0] == "d":
            t.delete(op[1])
        elif op[0] == "l":
            raw = bytes.fromhex(test["files"][op[1]])
            for i in range(0, len(raw) - 7, 8):
                t.put(int.from_bytes(raw[i:i + 4], "little", signed=True),
                      int.from_bytes(raw[i + 4:i + 8], "little", signed=True))
        elif op[0] == "g":
            v, _ = t.get(op[1])
            out.append("" if v == TOMB else str(v))
        elif op[0] == "r":
            out.append(" ".join(f"{k}:{v}" for k, v in t.range(op[1], op[2])))
    return out
