#!/usr/bin/env python3
"""Compare the kernels of two `make isa` outputs (csrc/Makefile: OUT/obj of
`make isa UNIT=... OUT=...` at two commits): per kernel the instruction stream
(comments and directives dropped, the kernel's own symbol replaced, block
labels renumbered) and the -Rpass-analysis=kernel-resource-usage lines.
Prints one line per kernel (same / DIFF, instruction lines, a digest of the
stream, registers, spills, LDS, occupancy) and the counts per unit.  Kernels
are paired by their mangled names; a k_part_apply whose last template
argument (LEAN) is false pairs with the parent's kernel that has no such
argument.
Usage: python tools/isa_cmp.py PARENT_OBJ NEW_OBJ UNIT..."""
import hashlib
import re
import shutil
import subprocess
import sys


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt:
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout
    return dict(zip(names, out.splitlines()))


def kernels(path):
    text = open(path).read().splitlines()
    symset = {l.split()[1] for l in text if l.strip().startswith(".amdhsa_kernel ")}
    bodies = {}
    cur = None
    for l in text:
        s = l.split(";")[0].rstrip()
        if not s.strip():
            continue
        m = re.match(r"^(\S+):\s*$", s)
        if m and m.group(1) in symset:
            cur = m.group(1)
            bodies[cur] = []
            continue
        if cur is None:
            continue
        st = s.strip()
        if st.startswith(".Lfunc_end"):
            cur = None
            continue
        if st.startswith(".") and not re.match(r"^\.LBB\d+_\d+:", st):
            continue  # a directive
        bodies[cur].append(st)
    norm = {}
    for k, lines in bodies.items():
        labels = {}
        body = []
        for l in lines:
            l = l.replace(k, "SELF")
            l = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), l)
            body.append(re.sub(r"\s+", " ", l))
        norm[k] = body
    return norm


def resources(path):
    res = {}
    cur = None
    for l in open(path):
        m = re.search(r"remark: [^ ]+ (.*)$", l.strip())
        if not m:
            continue
        t = m.group(1).replace(" [-Rpass-analysis=kernel-resource-usage]", "")
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            res[cur] = []
        elif cur is not None:
            res[cur].append(t.strip())
    return res


def without_lean(names, parent):
    """A k_part_apply of the new side whose last template argument, LEAN, is
    false, under the name it has at a parent that has no such parameter."""
    out = {}
    for k, v in names.items():
        old = re.sub(r"(k_part_applyI\w*?)Lb0E(EEvPKmPKjiijmPjmiPhNS_10StackTableE)$", r"\1\2", k)
        out[old if old != k and old in parent and k not in parent else k] = v
    return out


def main():
    pa, nb = sys.argv[1], sys.argv[2]
    tot = [0, 0, 0]
    for unit in sys.argv[3:]:
        ka = kernels(f"{pa}/{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
        kb = kernels(f"{nb}/{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
        ra = resources(f"{pa}/resource_usage_{unit}.txt")
        rb = resources(f"{nb}/resource_usage_{unit}.txt")
        kb, rb = without_lean(kb, ka), without_lean(rb, ka)
        differing = 0
        dm = demangle(sorted(set(ka) | set(kb)))
        print(f"== {unit}: kernels at the parent {len(ka)}, now {len(kb)}; "
              f"only at the parent {len(set(ka) - set(kb))}, only now {len(set(kb) - set(ka))}")
        for k in sorted(set(ka) - set(kb)):
            print("  ONLY PARENT", dm[k])
        for k in sorted(set(kb) - set(ka)):
            print("  ONLY NEW", dm[k])
        for k in sorted(set(ka) & set(kb), key=lambda x: dm[x]):
            same_isa = ka[k] == kb[k]
            same_res = ra.get(k) == rb.get(k) and ra.get(k) is not None
            if not (same_isa and same_res):
                differing += 1
            r = dict(x.split(":", 1) for x in ra.get(k, []) if ":" in x)
            name = re.sub(r"^void bloomhip::\(anonymous namespace\)::", "", dm[k]).split("(bloomhip::")[0]
            h = hashlib.sha256("\n".join(ka[k]).encode()).hexdigest()[:12]
            print(f"  {'same' if same_isa and same_res else 'DIFF isa=%s res=%s' % (same_isa, same_res)} "
                  f"{name}: {len(ka[k])} -> {len(kb[k])} lines, parent sha {h}; VGPRs{r.get('VGPRs', '?')} "
                  f"SGPRs{r.get('TotalSGPRs', '?')} spill{r.get('VGPRs Spill', '?')} "
                  f"LDS{r.get('LDS Size [bytes/block]', '?')} occ{r.get('Occupancy [waves/SIMD]', '?')}")
        print(f"== {unit}: differing {differing}")
        tot[0] += len(ka)
        tot[1] += len(kb)
        tot[2] += differing
    print(f"== total: parent {tot[0]}, now {tot[1]}, differing {tot[2]}")


if __name__ == "__main__":
    main()
