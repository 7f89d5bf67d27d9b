"""Which geometries get pass 1's software-pipelined tile loop (bloom_pass1.h
pass1_pipe, Pass1Kernel::pipe: a tile scattered inside the hash phase of the
workgroup's next tile) on a 256-CU device, through the micro-benchmark
library's ubench_pass1_pipe: no device call, no GPU.

The loop runs in the family that got the hash-phase priority, the 512-thread
builds on three workgroups per CU (packed and entry_t keys), on the
one-member ladder.  The same family's general remainder measured slower with
it (its pipelined kernel spills registers) and keeps the plain loop, as does
everything else: strided keys and m >= 2^32 (the large histogram, two
workgroups per CU), the probes with their slot plane, the 1024-thread builds
and the super-tiles.  The rows are worked out by hand from the kernel each
geometry gets (tests/test_host.py PASS1_ROWS: threads, slots, workgroups per
CU), not by running the rule.
"""
import ctypes
import os

import pytest

import bloomhip as bh

# (n keys, m bits, slots, key stride) -> pipe
ROWS = [
    # C2: 512 threads, no slots, three workgroups per CU; also from entry_t runs
    (16_777_216, 167_772_160, 0, 4, 1),
    (16_777_216, 167_772_160, 0, 8, 1),
    # the same family on fewer keys: m = 3 << 26 is the relabelled one-member
    # ladder (PASS1_ROWS: kModLadder0R)
    (1_000_000, 3 << 26, 0, 4, 1),
    (1_000_000, 3 << 26, 0, 8, 1),
    # the family's general remainder (m = 100,000,007: 255 segments at
    # capacity 511, three workgroups per CU; m = 100,000: one segment):
    # measured slower, the plain loop
    (1_000_000, 100_000_007, 0, 4, 0),
    (1_000_000, 100_000_007, 0, 8, 0),
    (100_000, 100_000, 0, 4, 0),
    # strided keys take the large histogram: 512 threads on two workgroups per CU
    (16_777_216, 167_772_160, 0, 12, 0),
    # m >= 2^32 (the wide remainder): the largest capacity, 1024 threads
    (1_000_000, 2**32, 0, 4, 0),
    # one 1024-thread workgroup per CU: C5, the f = 10 tree's level 2, the p2
    # build on 503 segments
    (67_108_864, 671_088_640, 0, 4, 0),
    (16_777_216, 512_000_000, 0, 4, 0),
    (1_000_000, 51 << 23, 0, 4, 0),
    # super-tiles (C4)
    (268_435_456, 3 << 30, 0, 4, 0),
    # probes: 512 threads at two workgroups per CU with the slot plane, 1024 threads
    (16_777_216, 3 << 26, 1, 4, 0),
    (16_777_216, 671_088_640, 1, 4, 0),
]


def _pipe(n, m, slots, stride):
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    ub = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    ub.ubench_pass1_pipe.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t,
                                     ctypes.c_int, ctypes.c_void_p]
    out = ctypes.c_int(-1)
    return ub.ubench_pass1_pipe(n, m, slots, stride, 256, ctypes.byref(out)), out.value


@pytest.mark.parametrize("n,m,slots,stride,want", ROWS)
def test_pass1_scatter_overlap_rule(n, m, slots, stride, want):
    assert _pipe(n, m, slots, stride) == (0, want)


def test_pass1_scatter_overlap_refusal():
    """No segment geometry for m = 2^40: refused before a kernel is chosen."""
    for slots in (0, 1):
        assert _pipe(1_000_000, 1 << 40, slots, 4) == (-34, -1)
