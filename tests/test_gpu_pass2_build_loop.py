"""The build's lean pass-2 loop (k_part_apply's LEAN: the one-vector group
walk on 32-bit offsets, its body written twice), forced on each geometry
through the micro-benchmark library's ubench_part_loop (the product's pass 1,
then pass 2 on the given loop) and compared bit-exactly with the C oracle.

A workgroup has Q = 256 lane groups at G = 4, group q walking tiles q, q + Q,
..., so the tile counts 1, 255, 256, 257, 512 and 513 (each ending in a short
tile of 777 keys) give groups with 0, 1, 2 and 3 tiles; with random keys the
runs of a tile's 256-505 segments take one to a few steps each, so groups end
a run and change tile on either half of the loop body.  The skewed batch (one
key repeated across a whole tile) has a run many steps long among empty ones,
the tiny batch (5 keys) nearly only empty runs.  The merge case ORs a second
batch into a built filter through the same loop, then builds afresh after a
clear.
"""
import ctypes
import os

import numpy as np
import pytest

import bloomhip as bh

pytestmark = pytest.mark.gpu

# plan_build's one-member ladder and segments with a general remainder (both
# on 4096-key tiles), segments on 8192-key tiles (m = 15625 << 15; 15625 << 14
# and below plan 4096-key tiles), the ladder on 8192-key tiles
GEOMETRIES = {"ladder": (5 << 23, 4096), "segments": (41_943_053, 4096), "tiles8192": (15625 << 15, 8192),
              "ladder8192": (5 << 27, 8192)}
SHAPES = [1, 255, 256, 257, 512, 513, "skew", "tiny"]
LEAN = 1


@pytest.fixture(scope="module")
def ub():
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    L = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    L.ubench_walk_choice.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_void_p]
    L.ubench_part_loop.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64] + \
        [ctypes.c_void_p] * 4 + [ctypes.c_size_t] * 2
    return L


def _geometry(torch, ub, m):
    """Tile keys and segments of the product's build into m bits on this device."""
    out = np.zeros(7, dtype=np.int32)
    size = np.array([m], dtype=np.uint64)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ub.ubench_walk_choice(1, 1, size.ctypes.data, cus, out.ctypes.data) == 0
    return int(out[1]), int(out[2])


def _keys(shape, tk, seed=0):
    rng = np.random.default_rng(tk + seed + (shape if isinstance(shape, int) else 7))
    if shape == "skew":
        keys = np.concatenate([np.full(tk, 12345, dtype=np.int32),
                               rng.integers(-2**31, 2**31, size=2 * tk + 777, dtype=np.int64).astype(np.int32),
                               np.full(tk + 5, -7, dtype=np.int32)])
        rng.shuffle(keys[tk:])
        return keys
    if shape == "tiny":
        return rng.integers(-2**31, 2**31, size=5, dtype=np.int64).astype(np.int32)
    return rng.integers(-2**31, 2**31, size=(shape - 1) * tk + 777, dtype=np.int64).astype(np.int32)


def _buffers(torch, ub, geometry, nkeys):
    """The geometry's m and tile size, and device buffers for nkeys keys."""
    m, want_tk = GEOMETRIES[geometry]
    tk, nbins = _geometry(torch, ub, m)
    assert tk == want_tk, (geometry, tk)
    ntiles = (nkeys + tk - 1) // tk
    return m, tk, dict(pos=torch.empty(ntiles * tk, dtype=torch.int64, device="cuda"),
                       runs=torch.empty(ntiles * (nbins + 1) * 2, dtype=torch.int32, device="cuda"),
                       words=torch.zeros((m + 63) // 64 * 2, dtype=torch.int32, device="cuda"))


def _run(torch, ub, buf, m, keys, merge):
    dk = torch.from_numpy(keys).cuda()
    s = torch.cuda.current_stream()
    rc = ub.ubench_part_loop(LEAN, merge, dk.data_ptr(), keys.size, m, buf["pos"].data_ptr(),
                             buf["runs"].data_ptr(), buf["words"].data_ptr(), s.cuda_stream,
                             buf["pos"].numel(), buf["runs"].numel())
    assert rc == 0, rc
    torch.cuda.synchronize()


def _want(torch, coracle, m, keys):
    return torch.from_numpy(coracle.build(m, keys).view(np.int32)).cuda()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_lean_loop_matches_oracle(ub, coracle, geometry, shape):
    torch = pytest.importorskip("torch")
    tk = GEOMETRIES[geometry][1]
    keys = _keys(shape, tk)
    m, _, buf = _buffers(torch, ub, geometry, keys.size)
    if isinstance(shape, int):
        assert (keys.size + tk - 1) // tk == shape
    _run(torch, ub, buf, m, keys, 0)
    assert torch.equal(buf["words"], _want(torch, coracle, m, keys))


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_lean_loop_merges_then_rebuilds(ub, coracle, geometry):
    torch = pytest.importorskip("torch")
    tk = GEOMETRIES[geometry][1]
    first, second = _keys(257, tk), _keys(3, tk, seed=99)
    m, _, buf = _buffers(torch, ub, geometry, first.size)
    _run(torch, ub, buf, m, first, 0)
    _run(torch, ub, buf, m, second, 1)  # ORed into the built filter
    assert torch.equal(buf["words"], _want(torch, coracle, m, np.concatenate([first, second])))
    buf["words"].zero_()  # clear(), then a fresh build
    _run(torch, ub, buf, m, second, 0)
    assert torch.equal(buf["words"], _want(torch, coracle, m, second))
