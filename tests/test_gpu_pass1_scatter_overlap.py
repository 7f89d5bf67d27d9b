"""Pass 1's software-pipelined tile loop (k_part_bin's PIPE): the 512-thread
builds on three workgroups per CU scatter a tile inside the hash phase of the
workgroup's next tile, on two alternating histograms, and scatter and write
out a block's last tile in an epilogue.  The loop is walked through every
shape of a block's rounds (the shapes and cached references of
test_gpu_pass1_pipeline, placed by the device's CU count, g = 3 x CU count
workgroups):
  only_short       the block's only tile is short: only the epilogue scatters;
  one_full_each    the peeled tile and the epilogue, no loop body;
  full_into_1key,
  full_into_short  a short tile hashed while a full one is scattered, then
                   scattered itself in the epilogue;
  three_rounds     one loop iteration;
  four_rounds      each histogram used twice;
  five_rounds      both histograms twice and an odd tail.
Each case first checks which loop its geometry gets; the build must then be
bit-exact against the C oracle: on the one-member ladder (m = 5 << 25 and the
p2 form 3 << 26, which a build relabels to a one-member ladder as well), both
pipelined, and on the general remainder (100,000,007), which keeps the plain
loop of the same family because the pipelined one measured slower there
(bloom_pass1.h pass1_pipe); from entry_t keys, and as a second batch merged
into a built filter.
"""
import ctypes
import os

import numpy as np
import pytest

import bloomhip as bh
from test_gpu_pass1_pipeline import counts_4096, cu_count, keys_of, partition_build, want_build

pytestmark = pytest.mark.gpu

CASES = ["only_short", "one_full_each", "full_into_1key", "full_into_short", "three_rounds",
         "four_rounds", "five_rounds"]
MS = {"ladder": 5 << 25, "p2": 3 << 26, "general": 100_000_007}
# the loop each m gets (tests/test_host.py PASS1_ROWS: kModLadder0R, kModLadder0R, kModFast)
PIPE = {5 << 25: 1, 3 << 26: 1, 100_000_007: 0}


def count_of(case):
    g = 3 * cu_count()
    more = {
        "four_rounds": 4096 * (3 * g + 5) + 17,  # a fourth round: each histogram twice
        "five_rounds": 4096 * (4 * g + 5) + 17,  # a fifth: the pair twice, then an odd tail
    }
    return more[case] if case in more else counts_4096()[case]


def pipe_of(n, m, stride):
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    ub = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    ub.ubench_pass1_pipe.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t,
                                     ctypes.c_int, ctypes.c_void_p]
    out = ctypes.c_int(-1)
    assert ub.ubench_pass1_pipe(n, m, 0, stride, cu_count(), ctypes.byref(out)) == 0
    return out.value


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("m", list(MS.values()), ids=list(MS))
def test_pipelined_build_matches_oracle(coracle, m, case):
    n = count_of(case)
    assert pipe_of(n, m, 4) == PIPE[m]
    f = partition_build(m, keys_of(n))
    assert (f.words() == want_build(coracle, m, n)).all()


@pytest.mark.parametrize("m", list(MS.values()), ids=list(MS))
def test_pipelined_build_from_entry_keys(coracle, m):
    """entry_t keys (stride 8, 16-B aligned): the family's KEYS_ENTRY kernels."""
    n = count_of("full_into_short")
    assert pipe_of(n, m, 8) == PIPE[m]
    aos = np.zeros((n, 2), dtype=np.int32)
    aos[:, 0] = keys_of(n)
    f = partition_build(m, aos.reshape(-1), n=n, stride=8)
    assert (f.words() == want_build(coracle, m, n)).all()


@pytest.mark.parametrize("m", list(MS.values()), ids=list(MS))
def test_pipelined_build_merges_second_batch(coracle, m):
    """A second batch of the same count ORed into a built filter."""
    n = count_of("full_into_short")
    assert pipe_of(n, m, 4) == PIPE[m]
    more = keys_of(n, seed=1)
    f = partition_build(m, keys_of(n))
    f.set_batch(more)
    want = want_build(coracle, m, n).copy()
    coracle.set_into(want, m, more)
    assert (f.words() == want).all()
