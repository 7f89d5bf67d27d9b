"""Pass 2's four group walks (k_part_apply's CHAINS, VECS, REDIR at G = 4),
each forced on each build geometry through the micro-benchmark library's
ubench_part_walk (the product's pass 1, then pass 2 on the given walk) and
compared bit-exactly with the C oracle.

A workgroup has Q = 256 lane groups at G = 4 and chain c of a group starts at
tile q + c Q, so the shapes are tile counts: 1, 256, 257 (the second chain's
first tile) and 513 (both chains advance once), each ending in a short tile of
777 keys, plus a skewed batch (one key repeated across a whole tile: a run
many steps long) mixed with random keys.  The walks are right at any run
length, so every (geometry, walk) pair must run.
"""
import ctypes
import os

import numpy as np
import pytest

import bloomhip as bh

pytestmark = pytest.mark.gpu

# plan_build's one-member ladder, segments, segments on super-tiles
GEOMETRIES = {"ladder": 5 << 23, "segments": 41_943_053, "super": 1_400_000_000}
WALKS = [(1, 1, 0), (1, 1, 1), (1, 2, 1), (2, 2, 1)]
SHAPES = [1, 256, 257, 513, "skew"]
_case = {}


@pytest.fixture(scope="module")
def ub():
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    L = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    L.ubench_walk_choice.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_void_p]
    L.ubench_part_walk.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64] + \
        [ctypes.c_void_p] * 4 + [ctypes.c_size_t] * 2
    yield L
    _case.clear()  # the last case's device buffers


def _geometry(torch, ub, m):
    """Tile keys and segments of the product's build into m bits on this device."""
    out = np.zeros(7, dtype=np.int32)
    size = np.array([m], dtype=np.uint64)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ub.ubench_walk_choice(1, 1, size.ctypes.data, cus, out.ctypes.data) == 0
    return int(out[1]), int(out[2])


def _keys(shape, tk):
    rng = np.random.default_rng(tk + (shape if shape != "skew" else 7))
    if shape == "skew":
        keys = np.concatenate([np.full(tk, 12345, dtype=np.int32),
                               rng.integers(-2**31, 2**31, size=2 * tk + 777, dtype=np.int64).astype(np.int32),
                               np.full(tk + 5, -7, dtype=np.int32)])
        rng.shuffle(keys[tk:])
        return keys
    return rng.integers(-2**31, 2**31, size=(shape - 1) * tk + 777, dtype=np.int64).astype(np.int32)


def _reference(torch, ub, coracle, geometry, shape):
    """Keys, buffers and the oracle's bitmap on the device for one (geometry,
    shape): made once, shared by the four walks (the last one is kept)."""
    if _case.get("key") != (geometry, shape):
        _case.clear()
        m = GEOMETRIES[geometry]
        tk, nbins = _geometry(torch, ub, m)
        keys = _keys(shape, tk)
        ntiles = (keys.size + tk - 1) // tk
        assert shape == "skew" or ntiles == shape
        want = torch.from_numpy(coracle.build(m, keys).view(np.int32)).cuda()
        _case.update(key=(geometry, shape), m=m, n=keys.size, want=want,
                     keys=torch.from_numpy(keys).cuda(),
                     pos=torch.empty(ntiles * tk, dtype=torch.int64, device="cuda"),
                     runs=torch.empty(ntiles * (nbins + 1) * 2, dtype=torch.int32, device="cuda"),
                     words=torch.empty_like(want))
    return _case


@pytest.mark.parametrize("walk", WALKS, ids=lambda w: "c%dv%dr%d" % w)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_forced_group_walk_matches_oracle(ub, coracle, geometry, shape, walk):
    torch = pytest.importorskip("torch")
    c = _reference(torch, ub, coracle, geometry, shape)
    c["words"].zero_()
    s = torch.cuda.current_stream()
    rc = ub.ubench_part_walk(*walk, c["keys"].data_ptr(), c["n"], c["m"], c["pos"].data_ptr(),
                             c["runs"].data_ptr(), c["words"].data_ptr(), s.cuda_stream,
                             c["pos"].numel(), c["runs"].numel())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.equal(c["words"], c["want"])
