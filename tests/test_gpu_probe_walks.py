"""Pass 2's walks in the probe modes (k_part_apply as kApplyProbe, kApplyStack,
kApplyLadder) at the tile counts where a walk's lane groups take a second
tile, through the public API and bit-exact against the C oracle.

One geometry per walk that launch_apply compiles for the probe modes:

* the segment stack on 16,384-key super-tiles, {G 4, CHAINS 1, VECS 2, REDIR};
* the segment stack on 8192-key tiles, {4, 1, 1, 0}; the same on strided
  workgroups (625 segments: a workgroup takes 2-3 of them); with eight members
  (the image that is never strided) on 4096-key tiles;
* the segment stack on short runs, {4, 1, 1, REDIR}: 6,144 segments of
  8192-key tiles (more than super-tiles sort), four entries per run;
* the segment stack's batch walk {8, 0, 1, 0}: 100 segments of 128 bits;
* the ladder, {8, 0, 1, 0}, members given largest and smallest first;
* the single partitioned probe's batch walks at G = 4 (4096- and 8192-key
  tiles), 8, 16 and 32.

A group walk's workgroup has Q = 256 lane groups at G = 4, group q taking tiles
q, q + Q, ...: 1, 255, 256, 257, 512 and 513 tiles.  The batch walk's 16 waves
take DEPTH * 64 / G tiles each and stride 16 batches on, so a workgroup's
second round starts past R = 2048 / G tiles: R - 1, R, R + 1, 2R and 2R + 1
tiles.  Every count ends in a short tile of 777 keys, the largest also in a
tile of one key.  The walks visit the tiles last to first, so a wrong clamp or
bound lands in tile 0 or in the short tile: every member's own keys are planted
in the first tile, the short tile, the first tile of the second round and the
middle one.  Tile keys and G come from the planners at test time.

Before each comparison the walk the planners choose on this device is asserted
(ubench_walk_choice / ubench_probe_walk_choice, no device call), and after the
call that exactly one stacked or partitioned pass ran, so neither another walk
nor a gather can stand in for the one under test.
"""
import ctypes
import functools
import os
import zlib

import numpy as np
import pytest

import bloomhip as bh

pytestmark = pytest.mark.gpu

PROBE, STACK, LADDER = 1, 2, 3  # bloom_pass2.h kApplyProbe, kApplyStack, kApplyLadder
C3 = [655_360 * 4**i for i in range(4, -1, -1)]
F10 = [512_000_000, 51_200_000, 5_120_000]

# name -> (member sizes in call order, the walk the planners must choose:
# mode, tile keys, G, CHAINS, VECS, REDIR)
GEOMETRIES = {
    "stack_super": (F10, (STACK, 16_384, 4, 1, 2, 1)),
    "stack_8192": ([51_200_000, 5_120_000], (STACK, 8192, 4, 1, 1, 0)),
    "stack_strided": ([256_000 * 10**i for i in (1, 2, 3)], (STACK, 8192, 4, 1, 1, 0)),
    "stack_redir": ([3 << 26, 1 << 15], (STACK, 8192, 4, 1, 1, 1)),
    "stack_eight": ([3 << 20, 1 << 20, 3 << 18, 1 << 18, 1 << 19, 3 << 17, 1 << 17, 1 << 16],
                    (STACK, 4096, 4, 1, 1, 0)),
    "stack_batch": ([12_800, 6_400, 3_200], (STACK, 4096, 8, 0, 1, 0)),
    "ladder": (C3, (LADDER, 8192, 8, 0, 1, 0)),
    "ladder_rev": (C3[::-1], (LADDER, 8192, 8, 0, 1, 0)),
    "probe_g4": ([5 << 25], (PROBE, 4096, 4, 0, 1, 0)),
    "probe_g4_8192": ([5 << 27], (PROBE, 8192, 4, 0, 1, 0)),
    "probe_g8": ([100_000], (PROBE, 4096, 8, 0, 1, 0)),
    "probe_g16": ([50_000], (PROBE, 4096, 16, 0, 1, 0)),
    "probe_g32": ([20_000], (PROBE, 4096, 32, 0, 1, 0)),
}
GROUP_SHAPES = [1, 255, 256, 257, 512, 513, "tail1"]
BATCH_SHAPES = ["R-1", "R", "R+1", "2R", "2R+1", "tail1"]
# one geometry per mode also from entry_t keys (stride 8), one tile into the second round
ENTRY_CASES = {("stack_super", 257), ("ladder", "R+1"), ("probe_g4", "R+1")}
SHORT_TILE = 777
PLANT = 90  # keys of each member per planted place: eight members fit the short tile
SLOTS = ("probe_stacked", "probe_stacked+route", "probe_partitioned", "k_probe", "k_probe_lds", "k_route")


def _is_group(geometry):
    return GEOMETRIES[geometry][1][3] != 0


CASES = [(g, s, stride) for g in GEOMETRIES for s in (GROUP_SHAPES if _is_group(g) else BATCH_SHAPES)
         for stride in ((4, 8) if (g, s) in ENTRY_CASES else (4,))]


@functools.lru_cache(maxsize=None)
def cu_count():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


_members = {}  # the last geometry's filters and oracle bitmaps
_want = {}     # the oracle's answers per (geometry, n), of the last geometry


@pytest.fixture(scope="module")
def ub():
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    L = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    L.ubench_walk_choice.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_void_p]
    L.ubench_probe_walk_choice.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    L.ubench_pass1_choice.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t,
                                      ctypes.c_int, ctypes.c_void_p]
    L.ubench_stack_pass1_choice.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    yield L
    _members.clear()
    _want.clear()


def walk_choice(ub, ms, n):
    """(mode, tile keys, segments, G, CHAINS, VECS, REDIR) of probing n keys
    against filters of ms bits on this device, from the planners."""
    out = np.zeros(7, dtype=np.int32)
    if len(ms) == 1:
        rc = ub.ubench_probe_walk_choice(n, ms[0], cu_count(), out.ctypes.data)
    else:
        sizes = np.array(sorted(ms, reverse=True), dtype=np.uint64)  # as probe_stacks orders them
        rc = ub.ubench_walk_choice(n, len(ms), sizes.ctypes.data, cu_count(), out.ctypes.data)
    assert rc == 0, rc
    return tuple(int(x) for x in out)


def pass1_choice(ub, ms, n, stride=4):
    """Pass1Kernel's fields (tests/test_host.py PASS1_ROWS) for the same probe."""
    out = np.zeros(11, dtype=np.int32)
    if len(ms) == 1:
        rc = ub.ubench_pass1_choice(n, ms[0], 1, stride, cu_count(), out.ctypes.data)
    else:
        sizes = np.array(sorted(ms, reverse=True), dtype=np.uint64)
        rc = ub.ubench_stack_pass1_choice(n, len(ms), sizes.ctypes.data, stride, cu_count(), out.ctypes.data)
    assert rc == 0, rc
    return tuple(int(x) for x in out)


def sorted_run(n, seed):
    rng = np.random.default_rng(seed)
    k = np.unique(rng.integers(-2**31, 2**31, size=n + n // 8 + 8, dtype=np.int64).astype(np.int32))
    return k[:n]


def members(coracle, geometry):
    """The geometry's filters (probed STACKED, or PARTITION when alone), each
    built as a run of about 40,000 sorted keys (fewer where that would fill a
    small filter with ones) with its run metadata, and per member the oracle's
    (keys, bitmap, m, fences, max key).  Built once per geometry."""
    if _members.get("geometry") != geometry:
        _members.clear()
        _want.clear()
        ms = GEOMETRIES[geometry][0]
        filters, refs = [], []
        for j, m in enumerate(ms):
            keys = sorted_run(int(min(40_000, max(64, m // 10))), 7000 + 10 * len(ms) + j)
            f = bh.BloomFilter(m)
            f.set_probe_strategy(bh.PROBE_PARTITION if len(ms) == 1 else bh.PROBE_STACKED)
            f.set_batch_run(keys)
            filters.append(f)
            fences, max_key = coracle.run_meta(keys)
            refs.append((keys, coracle.build(m, keys), m, fences, max_key))
        _members.update(geometry=geometry, filters=filters, refs=refs)
    return _members["filters"], _members["refs"]


def tile_count(shape, G, group):
    """Tiles of a shape; R: where a workgroup's second round starts."""
    R = 1024 // G if group else 2048 // G
    if isinstance(shape, int):
        return shape, R
    if shape == "tail1":
        return 2 * R + 1, R
    return {"R-1": R - 1, "R": R, "R+1": R + 1, "2R": 2 * R, "2R+1": 2 * R + 1}[shape], R


def probe_keys(geometry, refs, n, tk, R):
    """n random keys with PLANT keys of every member planted at the start of
    the first tile, of the last (short) tile, of the first tile of the second
    round (the walk goes last to first: data tile ntiles - 1 - R) and of the
    middle tile; in a one-key tile, one member's key."""
    rng = np.random.default_rng([zlib.crc32(geometry.encode()), n])
    keys = rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
    ntiles = (n + tk - 1) // tk
    places = sorted({0, ntiles - 1, max(ntiles - 1 - R, 0), ntiles // 2})
    for i, tile in enumerate(places):
        for j in range(len(refs)):
            src = refs[(i + j) % len(refs)][0]
            lo = min(tile * tk + j * PLANT, n)
            hi = min(lo + PLANT, n, (tile + 1) * tk)
            keys[lo:hi] = src[(i * PLANT + np.arange(hi - lo)) % src.size]
    return keys


def wanted(coracle, geometry, refs, n, tk, R):
    """The probe keys of (geometry, n) and the oracle's packed rows for them,
    computed once and left unchanged."""
    if (geometry, n) not in _want:
        keys = probe_keys(geometry, refs, n, tk, R)
        rows = np.stack([coracle.test(w, m, keys) for _, w, m, _, _ in refs])
        keys.setflags(write=False)
        rows.setflags(write=False)
        _want[(geometry, n)] = (keys, rows)
    return _want[(geometry, n)]


def launches_of(f0, call):
    """call()'s result and its launches per profile slot of SLOTS, recorded on
    f0 (the first handle of a multi-filter call)."""
    f0.profile(True)
    f0.profile_reset()
    try:
        out = call()
        prof = f0.profile_read()
    finally:
        f0.profile(False)
    return out, {s: prof[s]["launches"] for s in SLOTS if s in prof}


def as_entries(keys):
    aos = np.zeros((keys.size, 2), dtype=np.int32)
    aos[:, 0] = keys
    return aos.reshape(-1)


def check_probe(ub, coracle, geometry, n, R, stride=4):
    """test_batch of (geometry, n) against the oracle, the walk and the pass asserted."""
    ms, walk = GEOMETRIES[geometry]
    filters, refs = members(coracle, geometry)
    mode, tk, nbins, G, chains, vecs, redir = walk_choice(ub, ms, n)
    assert (mode, tk, G, chains, vecs, redir) == walk
    if geometry == "stack_strided":
        # more segments than resident workgroups (at most two per CU): stack_stride strides
        assert nbins > 2 * cu_count()
    keys, want = wanted(coracle, geometry, refs, n, tk, R)
    if stride == 8:
        got, ran = launches_of(filters[0], lambda: bh.test_batch(filters, as_entries(keys), n=n, stride=8))
    else:
        got, ran = launches_of(filters[0], lambda: bh.test_batch(filters, keys))
    assert ran == {"probe_partitioned" if len(ms) == 1 else "probe_stacked": 1}, ran
    for j in range(len(ms)):
        assert np.array_equal(got[j], want[j]), (geometry, n, j, ms[j])


def shape_keys(ub, geometry, shape):
    """(n keys, R) of a shape, tile keys and G from the planners."""
    ms, walk = GEOMETRIES[geometry]
    _, tk, _, G, chains, _, _ = walk_choice(ub, ms, 1)
    tiles, R = tile_count(shape, G, chains != 0)
    return (tiles - 1) * tk + (1 if shape == "tail1" else SHORT_TILE), R


@pytest.mark.parametrize("geometry,shape,stride", CASES,
                         ids=["%s-%s-%s" % (g, s, "entry" if st == 8 else "packed") for g, s, st in CASES])
def test_probe_walk_matches_oracle(ub, coracle, geometry, shape, stride):
    n, R = shape_keys(ub, geometry, shape)
    check_probe(ub, coracle, geometry, n, R, stride)


# ------------------------------------------------------------- routing ----
@pytest.mark.parametrize("layout", ["packed", "entry"])
@pytest.mark.parametrize("tiles", [257, 513])
@pytest.mark.parametrize("geometry", ["ladder", "stack_super"])
def test_route_on_walk_shapes(ub, coracle, geometry, tiles, layout):
    """route_gets_packed over the same members as runs (their metadata from
    set_batch_run): one stack takes every run, so the routing runs in the
    stack's combine (k_probe_combine_route), on a ragged second round."""
    ms, walk = GEOMETRIES[geometry]
    _, tk, _, G, chains, _, _ = walk_choice(ub, ms, 1)
    R = tile_count(tiles, G, chains != 0)[1]
    n = (tiles - 1) * tk + SHORT_TILE
    mode, tk2, _, G2, chains2, vecs, redir = walk_choice(ub, ms, n)
    assert (mode, tk2, G2, chains2, vecs, redir) == walk
    runs, refs = members(coracle, geometry)
    gets = probe_keys(geometry, refs, n, tk, R)
    gets[-4:] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, refs[0][0][0], refs[0][0][-1]]
    wc, wf, wp = coracle.route([(w, m, fences, mk) for _, w, m, fences, mk in refs], gets)
    want = np.where(wf < 0, np.uint32(bh.ROUTE_NONE),
                    (wf.astype(np.uint32) << np.uint32(bh.ROUTE_PAGE_BITS)) | wp.astype(np.uint32))
    if layout == "entry":
        (cand, route), ran = launches_of(
            runs[0], lambda: bh.route_gets_packed(runs, as_entries(gets), n=n, stride=8))
    else:
        (cand, route), ran = launches_of(runs[0], lambda: bh.route_gets_packed(runs, gets))
    assert ran == {"probe_stacked+route": 1}, ran
    assert (wf >= 0).sum() > PLANT  # the planted keys are routed somewhere
    assert np.array_equal(cand, wc)
    assert np.array_equal(route, want)


# -------------------------------------------------- pass 1, slot plane ----
@pytest.mark.parametrize("which", ["one_key_tail", "short_tail"])
def test_pass1_slot_plane_512_threads_second_tile(ub, coracle, which):
    """The probe's 512-thread pass 1 (4096-key tiles, two workgroups per CU, the
    slot plane) when a workgroup takes a second tile: 2C + 1 tiles ending in a
    one-key tile, 2C + 2 tiles ending in a tile of 4095 keys."""
    C = cu_count()
    ms, _ = GEOMETRIES["probe_g4"]
    n = {"one_key_tail": 2 * C * 4096 + 1, "short_tail": (2 * C + 1) * 4096 + 4095}[which]
    p = pass1_choice(ub, ms, n)
    # super, threads, layout, slots, ..., workgroups per CU (index 7), ..., grid (index 10)
    assert (p[0], p[1], p[3], p[7], p[10]) == (0, 512, 1, 2, 2 * C), p
    _, tk, _, G, _, _, _ = walk_choice(ub, ms, n)
    assert tk == 4096 and (n + tk - 1) // tk > p[10]
    check_probe(ub, coracle, "probe_g4", n, 2048 // G)


def test_pass1_slot_plane_super_tiles_second_tile(ub, coracle):
    """Pass 1 on super-tiles with the slot plane runs one workgroup per CU: on
    at most 256 CUs the 257- and 513-tile cases above give a workgroup a second
    and a third tile; on more, C + 1 tiles do, here."""
    C = cu_count()
    ms, _ = GEOMETRIES["stack_super"]
    for tiles in (257, 513, C + 1):
        p = pass1_choice(ub, ms, (tiles - 1) * 16_384 + SHORT_TILE)
        assert (p[0], p[1], p[3], p[7], p[10]) == (1, 1024, 1, 1, min(C, tiles)), p
    if C <= 256:
        assert min(C, 257) < 257  # test_probe_walk_matches_oracle[stack_super-257-*] took a second tile
    else:
        check_probe(ub, coracle, "stack_super", C * 16_384 + SHORT_TILE, 256)
