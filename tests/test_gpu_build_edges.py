"""The partition build with its write-through stores (pass 1's sorted tiles in
the pipelined family from packed keys, a fresh filter's bitmap on the
one-vector group walk), bit-exact against the C oracle.

- Product path (set_batch on the partition strategy) on plan_build's
  one-member ladder and on its segments: 5, 12, 13 and 17 whole tiles, 13
  tiles and a ragged 777 keys, and a skewed batch (one key fills a whole tile:
  a run many steps long, empty runs elsewhere); and around pass 2's walk,
  whose 256 lane groups take tiles q, q + 256, ...: exactly 256 tiles, 257 (one
  group advances to a second tile) and 513.  Each case builds a fresh
  filter, merges a second batch into it (the plain read-modify-write), then
  clears it and builds afresh: both write-backs.  Packed keys and entry_t keys
  at stride 8.  On the device's own grid these batches give a workgroup one
  tile at most, so:
- the same batches through ubench_part_grid on a forced grid of 6 on the
  ladder geometry m = 5 << 23: two whole rounds (12), a partial last round
  (13, 17), fewer tiles than workgroups (5), a ragged last tile, the skew;
  the pipelined loop's peeled tile, steady state and epilogue all store
  through the policy the product chooses, which the entry reports;
- one product-path batch on the device's own grid with a partial second round
  and a ragged end, n = grid * 4096 + (grid / 3) * 4096 + 777;
- the stamped kernels of the micro-benchmark library (tools/ubench.py edges),
  the same templates with the stamps compiled in: their bitmap equals the
  oracle's and a workgroup's stamps are in order.
"""
import ctypes
import os

import numpy as np
import pytest

import bloomhip as bh

pytestmark = pytest.mark.gpu

TK = 4096
GEOMETRIES = {"ladder": 5 << 23, "segments": 41_943_053}
SHAPES = [5, 12, 13, 17, "ragged13", "skew"]
# pass 2 walks a segment with Q = 256 lane groups, group q taking tiles q, q + Q, ...
WALK_SHAPES = [256, 257, 513]


def _keys(shape, seed):
    rng = np.random.default_rng(seed)
    rnd = lambda k: rng.integers(-2**31, 2**31, size=k, dtype=np.int64).astype(np.int32)  # noqa: E731
    if shape == "skew":
        return np.concatenate([np.full(TK, 12345, dtype=np.int32), rnd(2 * TK + 777),
                               np.full(TK + 5, -7, dtype=np.int32)])
    if shape == "ragged13":
        return rnd(13 * TK + 777)
    return rnd(shape * TK)


def _device_keys(torch, keys, stride):
    if stride == 4:
        return torch.from_numpy(keys).cuda()
    aos = np.zeros((keys.size, 2), dtype=np.int32)  # entry_t: key, value
    aos[:, 0] = keys
    aos[:, 1] = 0x5A5A5A5A
    return torch.from_numpy(aos.reshape(-1)).cuda()


@pytest.mark.parametrize("stride", [4, 8], ids=["packed", "entry"])
@pytest.mark.parametrize("shape", SHAPES + WALK_SHAPES)
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_build_merge_rebuild_match_oracle(coracle, geometry, shape, stride):
    torch = pytest.importorskip("torch")
    m = GEOMETRIES[geometry]
    a = _keys(shape, 11)
    b = _keys(shape if shape != 513 else 17, 12)
    da, db = _device_keys(torch, a, stride), _device_keys(torch, b, stride)
    f = bh.BloomFilter(m)
    f.set_strategy(bh.BUILD_PARTITION)
    f.set_batch(da, n=a.size, stride=stride)
    assert (f.words() == coracle.build(m, a)).all(), "fresh build"
    f.set_batch(db, n=b.size, stride=stride)
    assert (f.words() == coracle.build(m, np.concatenate([a, b]))).all(), "merge"
    f.clear()
    f.set_batch(db, n=b.size, stride=stride)
    assert (f.words() == coracle.build(m, b)).all(), "clear + fresh build"


@pytest.fixture(scope="module")
def ub():
    bh.lib()  # torch's HIP runtime first: one runtime per process
    L = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    L.ubench_part_grid.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64] + \
        [ctypes.c_void_p] * 4 + [ctypes.c_size_t] * 2
    L.ubench_part_geometry.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p]
    L.ubench_edges.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64] + [ctypes.c_void_p] * 4 + \
        [ctypes.c_size_t] * 2 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.ubench_edge_layout.argtypes = [ctypes.c_void_p]
    L.ubench_edge_layout.restype = None
    return L


@pytest.mark.parametrize("stride", [4, 8], ids=["packed", "entry"])
@pytest.mark.parametrize("shape", SHAPES)
def test_forced_grid_of_6_matches_oracle(ub, coracle, shape, stride):
    torch = pytest.importorskip("torch")
    m = GEOMETRIES["ladder"]
    a, b = _keys(shape, 21), _keys(shape, 22)
    n = max(a.size, b.size)
    geo = np.zeros(4, dtype=np.uint64)
    assert ub.ubench_part_geometry(n, m, geo.ctypes.data) == 0
    nbins, _, tk, ntiles = (int(x) for x in geo)
    assert tk == TK
    pos = torch.empty(ntiles * tk, dtype=torch.int64, device="cuda")
    runs = torch.empty(ntiles * (nbins + 1) * 2, dtype=torch.int32, device="cuda")
    words = torch.full(((m + 63) // 64 * 2,), -1, dtype=torch.int32, device="cuda")  # a fresh build overwrites
    s = torch.cuda.current_stream()

    def build(keys, merge):
        dk = _device_keys(torch, keys, stride)
        rc = ub.ubench_part_grid(6, int(stride == 8), merge, dk.data_ptr(), keys.size, m, pos.data_ptr(),
                                 runs.data_ptr(), words.data_ptr(), s.cuda_stream, pos.numel(), runs.numel())
        torch.cuda.synchronize()
        return rc
    # the pipelined loop; write-through tiles from packed keys, plain from entry_t
    assert build(a, 0) == (4 | (2 if stride == 4 else 0))
    assert torch.equal(words, torch.from_numpy(coracle.build(m, a).view(np.int32)).cuda()), "fresh build"
    assert build(b, 1) >= 0
    want = coracle.build(m, np.concatenate([a, b]))
    assert torch.equal(words, torch.from_numpy(want.view(np.int32)).cuda()), "merge"


def test_device_grid_partial_second_round_matches_oracle(coracle):
    torch = pytest.importorskip("torch")
    m = GEOMETRIES["ladder"]
    grid = 3 * torch.cuda.get_device_properties(0).multi_processor_count
    n = grid * TK + (grid // 3) * TK + 777
    keys = np.random.default_rng(31).integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
    f = bh.BloomFilter(m)
    f.set_strategy(bh.BUILD_PARTITION)
    f.set_batch(torch.from_numpy(keys).cuda(), n=n, stride=4)
    assert (f.words() == coracle.build(m, keys)).all()


def test_stamped_build_matches_oracle_and_stamps_are_ordered(ub, coracle):
    torch = pytest.importorskip("torch")
    L = ub
    m = 5 << 25  # the geometry the stamped kernels are compiled for
    keys = _keys("ragged13", 13)
    geo = np.zeros(4, dtype=np.uint64)
    assert L.ubench_part_geometry(keys.size, m, geo.ctypes.data) == 0
    nbins, _, tk, ntiles = (int(x) for x in geo)
    assert tk == TK and ntiles == 14
    lay = np.zeros(2, dtype=np.int32)
    L.ubench_edge_layout(lay.ctypes.data)
    S1, S2 = int(lay[0]), int(lay[1])  # u64 stamps per workgroup of pass 1, of pass 2
    assert S1 >= 5 and S2 == 5  # this batch: start, end, two tile stamps; pass 2's five stages
    dk = torch.from_numpy(keys).cuda()
    pos = torch.empty(ntiles * tk, dtype=torch.int64, device="cuda")
    runs = torch.empty(ntiles * (nbins + 1) * 2, dtype=torch.int32, device="cuda")
    words = torch.full(((m + 63) // 64 * 2,), -1, dtype=torch.int32, device="cuda")  # a fresh build overwrites
    stamps = torch.zeros(ntiles * S1 + nbins * S2, dtype=torch.int64, device="cuda")
    out4 = np.zeros(4, dtype=np.int32)
    s = torch.cuda.current_stream()
    rc = L.ubench_edges(dk.data_ptr(), keys.size, m, pos.data_ptr(), runs.data_ptr(), words.data_ptr(),
                        s.cuda_stream, pos.numel(), runs.numel(), stamps.data_ptr(), stamps.numel(),
                        out4.ctypes.data)
    assert rc == 0, rc
    torch.cuda.synchronize()
    want = torch.from_numpy(coracle.build(m, keys).view(np.int32)).cuda()
    assert torch.equal(words, want)
    g1, g2, rounds, khz = (int(x) for x in out4)
    assert (g1, g2, rounds) == (ntiles, nbins, 1) and khz > 0
    st = stamps.cpu().numpy()
    p1 = st[:g1 * S1].reshape(g1, S1)
    p2 = st[g1 * S1:].reshape(g2, S2)
    # pass 1: start, one loop iteration, the epilogue, the end; nothing else
    assert (p1[:, 0] > 0).all() and (p1[:, 4:] == 0).all()
    assert (p1[:, 0] <= p1[:, 2]).all() and (p1[:, 2] <= p1[:, 3]).all() and (p1[:, 3] <= p1[:, 1]).all()
    assert (np.diff(p2, axis=1) >= 0).all() and (p2[:, 0] > 0).all()
    assert p2[:, 0].min() >= p1[:, 1].max(), "pass 2 starts after pass 1's last workgroup"
