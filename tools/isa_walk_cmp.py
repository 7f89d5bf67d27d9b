#!/usr/bin/env python3
"""For the kernels that differ between two `make isa` outputs (tools/isa_cmp.py):
how many differing lines lie inside pass 2's walk loops (a loop with the
build's ds_or_b32 or the probes' result-byte stores and no s_barrier), and
whether those loops are the same instructions once registers are renamed by
their first use in the loop.
Usage: python tools/isa_walk_cmp.py PARENT_OBJ NEW_OBJ UNIT..."""
import sys, difflib, re
import os
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_cmp
pa, nb = sys.argv[1:3]
def walk_ranges(body):
    labels = {l[:-1]: k for k, l in enumerate(body) if re.match(r"^\.L\d+:$", l)}
    rs = []
    for k, l in enumerate(body):
        m = re.match(r"s_(?:cbranch_\w+|branch) (\.L\d+)$", l)
        if not m or m.group(1) not in labels or labels[m.group(1)] >= k: continue
        seg = body[labels[m.group(1)]:k + 1]
        if any(s.startswith("s_barrier") for s in seg): continue
        if any(s.startswith(("ds_or_b32", "global_store_byte", "global_store_short")) for s in seg):
            rs.append((labels[m.group(1)], k + 1))
    return rs
def inside(rs, a, b):
    return any(a < r1 and max(b, a + 1) > r0 for r0, r1 in rs)
for unit in sys.argv[3:]:
    ka = isa_cmp.kernels(f"{pa}/{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    kb = isa_cmp.kernels(f"{nb}/{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    dm = isa_cmp.demangle(sorted(ka))
    tot = bad = 0
    for k in sorted(ka, key=lambda x: dm[x]):
        if k not in kb or ka[k] == kb[k]: continue
        tot += 1
        ra, rb = walk_ranges(ka[k]), walk_ranges(kb[k])
        n_in = n_out = 0
        for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, ka[k], kb[k], autojunk=False).get_opcodes():
            if tag == "equal": continue
            n = max(i2 - i1, j2 - j1)
            if inside(ra, i1, i2) or inside(rb, j1, j2): n_in += n
            else: n_out += n
        name = re.sub(r"^void bloomhip::\(anonymous namespace\)::", "", dm[k]).split("(unsigned")[0]
        bad += n_in > 0
        print(f"  {name}: walk loops {len(ra)}/{len(rb)}, differing lines in walk loops {n_in}, outside {n_out}")
    print(f"== {unit}: differing {tot}, with a change inside a walk loop {bad}")

def canon(seg):
    names = {}
    def one(m):
        kind, a, b = m.group(1), m.group(2), m.group(3)
        if a is None:
            a = b = m.group(4)
        key = (kind, int(a))
        base = names.setdefault(key, len(names))
        return f"{kind}<{base}+{int(b) - int(a)}>"
    out = []
    for l in seg:
        l = re.sub(r"\.L\d+", ".L", l)
        out.append(re.sub(r"\b([vs])(?:\[(\d+):(\d+)\]|(\d+))\b", one, l))
    return out
print("-- walk-loop bodies with registers renamed by first use in the loop")
for unit in sys.argv[3:]:
    ka = isa_cmp.kernels(f"{pa}/{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    kb = isa_cmp.kernels(f"{nb}/{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    dm = isa_cmp.demangle(sorted(ka))
    same = diff = 0
    for k in sorted(ka, key=lambda x: dm[x]):
        if k not in kb or ka[k] == kb[k]: continue
        la = [canon(ka[k][a:b]) for a, b in walk_ranges(ka[k])]
        lb = [canon(kb[k][a:b]) for a, b in walk_ranges(kb[k])]
        if la == lb: same += 1
        else:
            diff += 1
            name = re.sub(r"^void bloomhip::\(anonymous namespace\)::", "", dm[k]).split("(unsigned")[0]
            print("  walk loops differ beyond register names:", name)
    print(f"== {unit}: differing kernels with walk loops equal up to register names {same}, not equal {diff}")
