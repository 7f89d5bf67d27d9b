"""Pass 1 with a phase priority (k_part_bin's PRIO): the 512-thread builds on
three workgroups per CU run their hash phase at s_setprio 1 and drop to 0 at
the post-rank barrier.  The priority changes which wave issues first, never a
result, so the builds must stay bit-exact against the C oracle through every
shape of a block's rounds (the shapes and cached references of
test_gpu_pass1_pipeline, placed by the device's CU count), on the one-member
ladder (m = 5 << 25), on the general remainder and from entry_t keys.  Each
case first checks that its geometry does get a kernel with a priority.
"""
import ctypes
import os

import numpy as np
import pytest

import bloomhip as bh
from test_gpu_pass1_pipeline import counts_4096, cu_count, keys_of, partition_build, want_build

pytestmark = pytest.mark.gpu

CASES = ["only_short", "full_into_1key", "full_into_short", "three_rounds"]


def prio_of(n, m, stride):
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    ub =ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    ub.ubench_pass1_prio.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t,
                                     ctypes.c_int, ctypes.c_void_p]
    out = ctypes.c_int(-1)
    assert ub.ubench_pass1_prio(n, m, 0, stride, cu_count(), ctypes.byref(out)) == 0
    return out.value


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("m", [5 << 25, 100_000_007], ids=["ladder", "general"])
def test_prioritised_build_matches_oracle(coracle, m, case):
    n = counts_4096()[case]
    assert prio_of(n, m, 4) != 0
    f = partition_build(m, keys_of(n))
    assert (f.words() == want_build(coracle, m, n)).all()


@pytest.mark.parametrize("m", [5 << 25, 100_000_007], ids=["ladder", "general"])
def test_prioritised_build_from_entry_keys(coracle, m):
    """entry_t keys (stride 8, 16-B aligned): the family's KEYS_ENTRY kernels."""
    n = counts_4096()["full_into_short"]
    assert prio_of(n, m, 8) != 0
    aos = np.zeros((n, 2), dtype=np.int32)
    aos[:, 0] = keys_of(n)
    f = partition_build(m, aos.reshape(-1), n=n, stride=8)
    assert (f.words() == want_build(coracle, m, n)).all()
