"""The issue priority of pass 1's phases per geometry (bloom_pass1.h
pass1_prio, Pass1Kernel::prio) on a 256-CU device, through the micro-benchmark
library's ubench_pass1_prio: no device call, no GPU.

PRIO is level | mode << 2 (modes: 0 the sort phases raised, 1 scatter and
packing, 2 the hash phase, 3 a static level for a workgroup's later waves).
Only the 512-thread builds that run three workgroups per CU measured faster
with one (the hash phase at level 1); every other family's kernels are
compiled with PRIO 0.  The rows are worked out by hand from the kernel each
geometry gets (tests/test_host.py PASS1_ROWS: threads, slots, workgroups per
CU), not by running the rule.
"""
import ctypes
import os

import pytest

import bloomhip as bh

HASH_1 = 1 | 2 << 2  # the hash phase at s_setprio 1

# (n keys, m bits, slots, key stride) -> prio
ROWS = [
    # C2: 512 threads, three workgroups per CU; also from entry_t runs
    (16_777_216, 167_772_160, 0, 4, HASH_1),
    (16_777_216, 167_772_160, 0, 8, HASH_1),
    # the same kernel family on fewer keys, and on the general remainder
    # (98 segments) at capacity 511: three workgroups per CU as well
    (1_000_000, 3 << 26, 0, 4, HASH_1),
    (100_000, 100_000, 0, 4, HASH_1),
    # strided keys take the large histogram: two workgroups per CU, not measured
    (16_777_216, 167_772_160, 0, 12, 0),
    # one 1024-thread workgroup per CU: C5, the f = 10 tree's level 2
    (67_108_864, 671_088_640, 0, 4, 0),
    (16_777_216, 512_000_000, 0, 4, 0),
    # super-tiles (C4)
    (268_435_456, 3 << 30, 0, 4, 0),
    # probes: 512 threads at two workgroups per CU, 1024 threads
    (16_777_216, 3 << 26, 1, 4, 0),
    (16_777_216, 671_088_640, 1, 4, 0),
]


def _prio(n, m, slots, stride):
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    ub = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    ub.ubench_pass1_prio.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t,
                                     ctypes.c_int, ctypes.c_void_p]
    out = ctypes.c_int(-1)
    return ub.ubench_pass1_prio(n, m, slots, stride, 256, ctypes.byref(out)), out.value


@pytest.mark.parametrize("n,m,slots,stride,want", ROWS)
def test_pass1_priority_rule(n, m, slots, stride, want):
    assert _prio(n, m, slots, stride) == (0, want)


def test_pass1_priority_refusal():
    """No segment geometry for m = 2^40: refused before a kernel is chosen."""
    for slots in (0, 1):
        assert _prio(1_000_000, 1 << 40, slots, 4) == (-34, -1)
