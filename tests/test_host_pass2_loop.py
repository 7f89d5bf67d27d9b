"""The host rule for pass 2's lean build loop (bloom_pass2.h choose_apply_walk,
ApplyWalk::lean): the builds on the one-vector group walk whose tiles come
from the Infinity Cache get it (C2, the f = 10 build, the general remainder),
and nothing else does.  No device call: the geometry comes from the
micro-benchmark library's ubench_walk_choice on a 256-CU device, the walk from
ubench_apply_walk (choose_apply_walk itself).
"""
import ctypes
import os

import numpy as np
import pytest

import bloomhip as bh

BUILD, PROBE, STACK, LADDER, BUILD_L = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def ub():
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    L = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    L.ubench_walk_choice.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_void_p]
    L.ubench_apply_walk.argtypes = [ctypes.c_int] + [ctypes.c_size_t] * 3 + [ctypes.c_void_p]
    return L


def _walk(ub, mode, tile_keys, nbins, ntiles):
    out = np.zeros(6, dtype=np.int32)
    ub.ubench_apply_walk(mode, tile_keys, nbins, ntiles, out.ctypes.data)
    return tuple(int(x) for x in out)


def _planned(ub, n, ms):
    """(mode, tile keys, segments, tiles) of the product's plan, then its walk."""
    sizes = np.array(ms, dtype=np.uint64)
    out = np.zeros(7, dtype=np.int32)
    assert ub.ubench_walk_choice(n, len(ms), sizes.ctypes.data, 256, out.ctypes.data) == 0
    mode, tk, nbins = int(out[0]), int(out[1]), int(out[2])
    return (mode, tk, nbins), _walk(ub, mode, tk, nbins, (n + tk - 1) // tk)


# (n keys, filter sizes) -> (mode, tile keys, segments), (G, CHAINS, VECS, REDIR, LEAN, offsets fit)
ROWS = [
    # the lean loop: C2, the f = 10 build, the general remainder (m = 100,000,007),
    # and C5's geometry at exactly the Infinity Cache's 256 MiB of tiles
    (16_777_216, [5 << 25], (BUILD_L, 4096, 256), (4, 1, 1, 0, 1, 1)),
    (16_777_216, [512_000_000], (BUILD, 8192, 505), (4, 1, 1, 0, 1, 1)),
    (16_777_216, [100_000_007], (BUILD, 4096, 255), (4, 1, 1, 0, 1, 1)),
    (33_554_432, [5 << 27], (BUILD_L, 8192, 512), (4, 1, 1, 0, 1, 1)),
    # entries from HBM (C5, and one tile past the Infinity Cache): two vectors
    (67_108_864, [5 << 27], (BUILD_L, 8192, 512), (4, 1, 2, 1, 0, 1)),
    (33_554_433, [5 << 27], (BUILD_L, 8192, 512), (4, 1, 2, 1, 0, 1)),
    # short runs: the redirected walk (m = 2^32; the ladder 5 << 29)
    (1_000_000, [2**32], (BUILD, 8192, 3277), (4, 1, 1, 1, 0, 1)),
    (1_000_000, [5 << 29], (BUILD_L, 8192, 2048), (4, 1, 1, 1, 0, 1)),
    # super-tiles: C4's two chains, and the one-vector walk on 2,048 segments
    (268_435_456, [3 << 30], (BUILD, 16_384, 2458), (4, 2, 2, 1, 0, 0)),
    (1_000_000, [2_684_354_559], (BUILD, 16_384, 2048), (4, 1, 1, 0, 0, 1)),
    # longer runs: the batch walk
    (100_000, [100_000], (BUILD, 4096, 98), (8, 0, 1, 0, 0, 1)),
    # probes: the segment stacks and the ladder
    (16_777_216, [512_000_000, 51_200_000, 5_120_000], (STACK, 16_384, 1250), (4, 1, 2, 1, 0, 1)),
    (16_777_216, [51_200_000, 5_120_000], (STACK, 8192, 320), (4, 1, 1, 0, 0, 1)),
    (16_777_216, [655_360 * 4 ** i for i in range(4, -1, -1)], (LADDER, 8192, 256), (8, 0, 1, 0, 0, 1)),
]


@pytest.mark.parametrize("n,ms,plan,walk", ROWS)
def test_lean_loop_choice(ub, n, ms, plan, walk):
    assert _planned(ub, n, ms) == (plan, walk)


def test_probe_modes_never_get_the_lean_loop(ub):
    """C2's geometry in every probe mode: the single probe's batch walk, the
    stack's group walk, the ladder's batch walk."""
    for mode in (PROBE, STACK, LADDER):
        assert _walk(ub, mode, 4096, 256, 4096)[4] == 0
    assert _walk(ub, BUILD, 4096, 256, 4096)[4] == 1


def test_offset_limit(ub):
    """The lean loop's tile offset is a signed 32-bit byte offset that steps
    512 tiles past the batch, its bounds a 32-bit offset into the run table:
    a batch of 2^31 bytes of either is refused, one below is taken.  (Every
    batch of tiles within the 256 MiB Infinity Cache fits, so the product's
    builds reach the limit only through the entries-from-HBM rule, which
    comes first.)"""
    tiles_4k = (1 << 31) // (4096 * 8) - 512  # tiles + 512 = 2^31 bytes
    assert _walk(ub, BUILD, 4096, 256, tiles_4k - 1)[5] == 1
    assert _walk(ub, BUILD, 4096, 256, tiles_4k)[5] == 0
    tiles_8k = (1 << 31) // (8192 * 8) - 512
    assert _walk(ub, BUILD, 8192, 505, tiles_8k - 1)[5] == 1
    assert _walk(ub, BUILD, 8192, 505, tiles_8k)[5] == 0
    # the run table: (segments + 1) * tiles * 4 bytes (on tiles small enough
    # that the table reaches 2^31 bytes before the tiles do)
    assert _walk(ub, BUILD, 64, 511, (1 << 31) // (512 * 4) - 1)[5] == 1
    assert _walk(ub, BUILD, 64, 511, (1 << 31) // (512 * 4))[5] == 0
    # past the limit (necessarily past the Infinity Cache) the walk is not the lean one
    assert _walk(ub, BUILD, 4096, 256, tiles_4k)[4] == 0
    assert _walk(ub, BUILD, 8192, 505, tiles_8k)[4] == 0
