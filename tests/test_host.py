"""Host-side checks of the engine library (CPU only, no kernel launches).

* libbloomhip.so loads and exports every symbol include/*.h declares;
* the kernels' position arithmetic (bloom_math.h, evaluated on the host via
  bloomhip_host_positions) equals the oracle for edge and random m;
* Run::Run sizing (bloomhip_m_bits) and argument validation;
* the workload generator restatement against independent RNGs.
"""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import bloomhip as bh
from bloom_oracle import np_m_bits, np_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    syms = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        text = open(h).read()
        syms.update(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(bloomhip_\w+)\s*\(", text, re.M))
    return sorted(syms)


def test_library_exports_every_declared_symbol():
    syms = _declared_symbols()
    assert len(syms) >= 25
    L = ctypes.CDLL(bh.LIB_PATH)
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing
    assert set(syms) == set(bh.EXPORTED_SYMBOLS)


def test_abi_version():
    assert bh.lib().bloomhip_abi_version() == 1


EDGE_M = [1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 65_536, 524_288, 1_000_003,
          655_360, 167_772_160, 671_088_640, 2**31 - 1, 2**31, 2**31 + 1, 3_221_225_472,
          2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**33 + 5, 2**46]


@pytest.fixture(scope="module")
def fuzz_keys():
    rng = np.random.default_rng(11)
    k = rng.integers(-2**31, 2**31, size=40_000, dtype=np.int64).astype(np.int32)
    k[:8] = [0, -1, 1, 2**31 - 1, -2**31, -2**31 + 1, 13141, -2_652_462]
    return k


@pytest.mark.parametrize("m", EDGE_M)
def test_engine_mod_arithmetic_edge_m(m, fuzz_keys):
    assert (bh.host_positions(m, fuzz_keys) == np_positions(fuzz_keys, m)).all()


def test_engine_mod_arithmetic_random_m(fuzz_keys):
    rng = np.random.default_rng(5)
    ms = np.concatenate([rng.integers(1, 2**32, size=300), rng.integers(1, 2**20, size=100),
                         (rng.integers(1, 64, size=50) << rng.integers(0, 26, size=50))])
    for m in ms.tolist():
        assert (bh.host_positions(int(m), fuzz_keys[:2000]) ==
                np_positions(fuzz_keys[:2000], int(m))).all(), m


def test_m_bits_matches_reference_sizing():
    rng = np.random.default_rng(2)
    for size, bpe in [(16_777_217, 10.0), (33_554_431, 0.5), (51_200, 7.7), (512, 0.5)] + [
            (int(s), float(np.float32(b))) for s, b in zip(rng.integers(1, 2**31, 200),
                                                          rng.uniform(0.1, 20, 200))]:
        assert bh.m_bits(size, bpe) == np_m_bits(size, bpe)


@pytest.mark.parametrize("size,bpe", [(512, 0.001), (0, 10.0), (100, -1.0), (100, float("nan"))])
def test_m_bits_rejects_empty_filter(size, bpe):
    with pytest.raises(bh.BloomHipError) as e:
        bh.m_bits(size, bpe)
    assert e.value.status == bh.EINVAL


def test_create_rejects_zero_bits():
    h = ctypes.c_void_p()
    assert bh.lib().bloomhip_create(0, 0, ctypes.byref(h)) == bh.EINVAL


def test_null_arguments_rejected():
    L = bh.lib()
    assert L.bloomhip_size(None, None) == bh.EINVAL
    assert L.bloomhip_set_batch(None, None, 0, 4, 0, None) == bh.EINVAL
    assert L.bloomhip_test_batch(None, 1, None, 0, 4, 0, None, 0, None) == bh.EINVAL
    assert L.bloomhip_destroy(None) == bh.EINVAL
    assert L.bloomhip_host_positions(0, None, 0, None) == bh.EINVAL


def test_no_gpu_fails_loudly_not_silently():
    """Without a device the engine must refuse, never fall back to the CPU."""
    if bh.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(bh.BloomHipError) as e:
        bh.BloomFilter(1024)
    assert e.value.status in (bh.ENODEV, bh.EIO)


def test_mt19937_matches_numpy():
    for seed in (13141, 13142, 0, 5489):
        ref = np.random.RandomState(seed if seed else 4357).randint(
            0, 2**32, size=3000, dtype=np.uint64).astype(np.uint32)
        assert (bh.gen_mt19937(seed, 3000) == ref).all()


def test_glibc_rand_matches_libc():
    libc = ctypes.CDLL("libc.so.6")
    for seed in (1, 2, 13141):
        libc.srand(seed)
        ref = np.array([libc.rand() for _ in range(4000)], dtype=np.int32)
        assert (bh.gen_glibc_rand(seed, 4000) == ref).all()
    libc.srand(1)


def test_puts_stream_is_even_mt_outputs():
    keys, vals = bh.gen_puts(13141, 1000, with_vals=True)
    mt = bh.gen_mt19937(13141, 2000).view(np.int32)
    assert (keys == mt[0::2]).all() and (vals == mt[1::2]).all()


def test_workload_small_stream_shape():
    puts, gets = bh.gen_workload(13141, 5000, 3000, 0.2, 0.3)
    assert puts.size == 5000 and gets.size == 3000
    # A puts-only prefix of the MT stream: puts draw key,value; miss-GETs draw
    # one value, so every put key is an MT output.
    mt = set(bh.gen_mt19937(13141, 20000).view(np.int32).tolist())
    assert set(puts.tolist()) <= mt
    # ~70% of non-repeated GETs come from earlier puts (miss ratio 0.3).
    frac = np.isin(gets, puts).mean()
    assert 0.55 < frac < 0.85


def test_c1_run_is_sorted_distinct_prefix():
    from bloomhip import workloads as W
    run, m = W.c1_run()
    assert m == 512_000 and run.shape == (51_200, 2)
    assert (np.diff(run[:, 0].astype(np.int64)) > 0).all()


def test_load_of_a_non_filter_file_fails_before_touching_the_gpu(tmp_path):
    """bloomhip_load validates the file on the host first (no GPU needed)."""
    import ctypes
    p = tmp_path / "junk.bloom"
    p.write_bytes(b"not a filter at all" * 10)
    h = ctypes.c_void_p()
    L = bh._lib()
    assert L.bloomhip_load(str(p).encode(), 0, ctypes.byref(h)) == bh.EINVAL
    assert L.bloomhip_load(str(tmp_path / "none").encode(), 0, ctypes.byref(h)) == -5  # EIO
    assert not h.value


def test_load_rejects_oversized_header_without_allocating(tmp_path):
    """A header whose sizes disagree with the file (here: 2^46 bits and 2^32-1
    fences in a 48-byte file) is refused before anything is sized from it."""
    import ctypes
    import struct
    L = bh._lib()
    h = ctypes.c_void_p()
    for m, nf in [((1 << 46), 0xFFFFFFFF), ((1 << 62), 0), (1000, 5)]:
        hdr = b"BLOOMHP1" + struct.pack("<IIQQIi", 1, 1, m, (m + 63) // 64, nf, 0)
        p = tmp_path / f"big_{m}_{nf}.bloom"
        p.write_bytes(hdr + b"\0" * 8)
        assert L.bloomhip_load(str(p).encode(), 0, ctypes.byref(h)) == bh.EINVAL
        assert not h.value


def test_binding_refuses_keys_that_are_not_int32():
    """Keys are KEY_t = int32 (src/types.h:4): an int64 array read as int32
    words would build the wrong keys, so the binding converts integer arrays
    at stride 4 (when they fit) and refuses anything else."""
    ptr, on_dev, keep = bh._keys_ptr(np.arange(10), 4)  # numpy's default int64
    assert keep.dtype == np.int32 and list(keep) == list(range(10)) and on_dev == 0
    with pytest.raises(ValueError):
        bh._keys_ptr(np.array([2**31]), 4)          # out of range
    with pytest.raises(ValueError):
        bh._keys_ptr(np.zeros((4, 2), dtype=np.int64), 8)  # int64 entries at stride 8
    with pytest.raises(ValueError):
        bh._keys_ptr(np.zeros(4, dtype=np.float32), 4)
    _, _, keep = bh._keys_ptr(np.zeros(8, dtype=np.int32), 8)
    assert bh._key_count(keep, 8, None) == 4
    with pytest.raises(ValueError):
        bh._key_count(keep, 8, 5)                  # 5 keys at stride 8 need 36 bytes
    with pytest.raises(ValueError):
        bh._out_ptr(np.zeros(3, dtype=np.uint64), 32, 8, "out")   # too small
    with pytest.raises(ValueError):
        bh._out_ptr(np.zeros(8, dtype=np.int32), 16, 8, "out")    # wrong element size
    with pytest.raises(ValueError):
        bh.compact([np.zeros((4, 2), dtype=np.int64)])


P2_D = (3, 5, 15, 17, 51, 85, 255)


def test_engine_p2_mod_every_form(fuzz_keys):
    """The p2 remainder (bloom_math.h mod_p2: m = d << t with d | 255, the
    byte-sum congruence and one multiply-high) against the exact remainder
    for every d and t it takes, and the m either side of each (general path)."""
    checked = 0
    for d in P2_D:
        for t in range(12, 32):
            m = d << t
            if m >= 2**32:
                continue
            for mm in (m, m - 1, m + 1):
                assert (bh.host_positions(mm, fuzz_keys[:4000]) ==
                        np_positions(fuzz_keys[:4000], mm)).all(), (d, t, mm)
            checked += 1
    assert checked > 100


def test_engine_wide_mod_random_m(fuzz_keys):
    """mod_wide (2^32 <= m <= 2^46: double-estimated quotient + one exact
    correction) against the exact remainder, m spread over the whole range
    and packed near powers of two and near quotient boundaries."""
    rng = np.random.default_rng(17)
    ms = np.concatenate([rng.integers(2**32, 2**46 + 1, size=200, dtype=np.uint64),
                         (np.uint64(1) << rng.integers(32, 47, size=60).astype(np.uint64)) +
                         rng.integers(-3, 4, size=60).astype(np.int64).astype(np.uint64),
                         np.array([2**32, 2**32 + 1, 2**32 + 1_000_003, 2**46, 2**46 - 1],
                                  dtype=np.uint64)])
    for m in ms.tolist():
        if not 2**32 <= m <= 2**46:
            continue
        assert (bh.host_positions(int(m), fuzz_keys[:3000]) ==
                np_positions(fuzz_keys[:3000], int(m))).all(), m


def test_library_is_built_from_these_kernel_sources():
    # the in-tree library carries the digest of the kernel sources it was
    # compiled from: a stale lib/ (sources edited, not rebuilt) fails here
    # before any GPU run measures the wrong kernels
    import hashlib
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    h = hashlib.sha256()
    for name in bench.kernel_sources():
        with open(os.path.join(root, "cs265-lsm-tree_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    assert bh.lib().bloomhip_kernel_sha().decode() == h.hexdigest()[:16]


def test_digest_covers_every_kernel_source():
    """csrc/Makefile's KERNEL_SRCS (the digest compiled into the library, read
    by bench.kernel_sources) lists every device source and header of the
    product: a kernel unit left out would change without changing the digest."""
    import glob
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    csrc = os.path.join(root, "cs265-lsm-tree_amd", "csrc")
    listed = bench.kernel_sources()
    assert len(set(listed)) == len(listed)
    for name in listed:
        assert os.path.exists(os.path.join(csrc, name)), name
    product = {os.path.basename(p) for p in glob.glob(os.path.join(csrc, "bloom_*"))
               if p.endswith((".hip", ".h"))}
    assert product <= set(listed), product - set(listed)
    assert "bloom_capi.cpp" in listed


@pytest.mark.parametrize("shift", [31, 32])
def test_planner_magic_bound_implies_exact(shift):
    """The planners (bloom_kernels.hip seg_magic, plan_ladder's computed
    tuple) skip their exhaustive check of a multiply-high divisor when
    x * e < 2^shift for every x they divide (M = ceil(2^shift / g),
    e = M g - 2^shift): the bound is checked here against brute force over
    every x it admits, for random and edge divisors."""
    rng = np.random.default_rng(7)
    gs = [1, 2, 3, 5, 7, 640, 4095, 4096, 40961, (1 << 20) - 1] + list(rng.integers(1, 1 << 22, 40))
    for g in gs:
        g = int(g)
        M = ((1 << shift) + g - 1) // g
        e = M * g - (1 << shift)
        xmax = (1 << shift) // e if e else 1 << 22  # x e < 2^shift for x < xmax
        xmax = min(xmax, 1 << 22)
        x = np.arange(xmax, dtype=np.uint64)
        got = (x * np.uint64(M)) >> np.uint64(32)
        want = x // np.uint64(2 * g) if shift == 31 else x // np.uint64(g)
        assert np.array_equal(got, want), g


# Pass 2's walk per geometry (bloom_pass2.h choose_apply_walk) on a 256-CU
# device, through the micro-benchmark library's ubench_walk_choice (no device
# call).  Rows: (n keys, filter sizes: one = a build, several = a stacked
# probe) -> (mode, tile keys, segments, G, CHAINS, VECS, REDIR).  C2 and C5
# are the kernels recorded in profiles/pass1_overlap/kernel_stats_c2_A.csv and
# kernel_stats_c5_A.csv; the others were read by hand off the planners and the
# launchers as they stood before the choice became one function.
BUILD, PROBE, STACK, LADDER, BUILD_L = 0, 1, 2, 3, 4
WALK_ROWS = [
    # C2, C5 run, C4
    (16_777_216, [167_772_160], (BUILD_L, 4096, 256, 4, 1, 1, 0)),
    (67_108_864, [671_088_640], (BUILD_L, 8192, 512, 4, 1, 2, 1)),
    (268_435_456, [3 << 30], (BUILD, 16_384, 2458, 4, 2, 2, 1)),
    # the f = 10 tree: level 2's build (505 segments of 8192-key tiles), the
    # three-level stack on super-tiles (1,250 segments), two levels (320)
    (16_777_216, [512_000_000], (BUILD, 8192, 505, 4, 1, 1, 0)),
    (16_777_216, [512_000_000, 51_200_000, 5_120_000], (STACK, 16_384, 1250, 4, 1, 2, 1)),
    (16_777_216, [51_200_000, 5_120_000], (STACK, 8192, 320, 4, 1, 1, 0)),
    # C3's five-level ladder: the batch walk at G = 8
    (16_777_216, [655_360 * 4 ** i for i in range(4, -1, -1)], (LADDER, 8192, 256, 8, 0, 1, 0)),
    # segment builds with runs of 96 / 192 / 384 entries and more: batch walk, G = 8 / 16 / 32
    (100_000, [100_000], (BUILD, 4096, 98, 8, 0, 1, 0)),
    (100_000, [50_000], (BUILD, 4096, 49, 16, 0, 1, 0)),
    (100_000, [20_000], (BUILD, 4096, 20, 32, 0, 1, 0)),
    # runs of 24 entries against 23: super-tile builds on 2,048 and 2,049
    # segments; 7-entry runs on 8192-key tiles (m = 2^32: 3,277 segments);
    # 12-entry runs on the one-member ladder 5 << 29 (2,048 bins)
    (1_000_000, [2_684_354_559], (BUILD, 16_384, 2048, 4, 1, 1, 0)),
    (1_000_000, [2_684_354_561], (BUILD, 16_384, 2049, 4, 2, 2, 1)),
    (1_000_000, [2**32], (BUILD, 8192, 3277, 4, 1, 1, 1)),
    (1_000_000, [5 << 29], (BUILD_L, 8192, 2048, 4, 1, 1, 1)),
    # sorted entries of exactly the Infinity Cache's 256 MiB (4,096 tiles of
    # 8192 keys) against one tile more, on C5's geometry
    (33_554_432, [671_088_640], (BUILD_L, 8192, 512, 4, 1, 1, 0)),
    (33_554_433, [671_088_640], (BUILD_L, 8192, 512, 4, 1, 2, 1)),
    # The stacks of tests/test_gpu_probe_walks.py, 513 tiles ending in 777 keys
    # (no member set is a ladder: the odd parts differ or are no divisor of 255).
    # 256,000 * 10^i, i = 1..3: m_max = 2^14 * 5^6, three members share 160 KiB:
    # w <= 436,906 bits, and the widest divisor of m_max that is a multiple of
    # 128 is 2^14 * 25 = 409,600: 625 segments, 8192-key tiles, runs of 39.
    (4_195_081, [256_000_000, 25_600_000, 2_560_000], (STACK, 8192, 625, 4, 1, 1, 0)),
    # 3 << 26 with 1 << 15: w <= the smallest member, so w = 2^15 and 6,144
    # segments, more than super-tiles sort (4,095): 8192-key tiles, runs of 4
    # entries, the short-run walk with the redirect
    (4_195_081, [3 << 26, 1 << 15], (STACK, 8192, 6144, 4, 1, 1, 1)),
    # eight members under 3 << 20: w <= 2^16, the widest w with a segment per
    # CU is 3 << 12 (256 segments): 4096-key tiles, runs of 48
    (2_097_929, [3 << 20, 1 << 20, 3 << 18, 1 << 18, 1 << 19, 3 << 17, 1 << 17, 1 << 16],
     (STACK, 4096, 256, 4, 1, 1, 0)),
    # 12,800 = 100 * 128 bits: even the narrowest w, 128 bits, gives fewer
    # segments than CUs, so that one: 100 segments, runs of 122 on 4096-key
    # tiles, the batch walk at G = 8
    (2_097_929, [12_800, 6_400, 3_200], (STACK, 4096, 100, 8, 0, 1, 0)),
]

# The same for a one-filter partitioned probe (ubench_probe_walk_choice:
# plan_segments, choose_tile_keys, choose_apply_walk(kApplyProbe)): always the
# batch walk, G from the run length 3 * tile keys / segments.  Rows: (n keys, m)
# -> as above.  5 << 25: 256 segments of 4096-key tiles, runs of 48; 5 << 27:
# 512 segments (PASS1_ROWS' C5 probe) of 8192-key tiles, runs of 48; 100,000 /
# 50,000 / 20,000 bits: 98 / 49 / 20 segments of 1,024 bits (the builds'
# rows above), runs of 125 / 250 / 614.
PROBE_WALK_ROWS = [
    (4_195_081, 5 << 25, (PROBE, 4096, 256, 4, 0, 1, 0)),
    (8_389_385, 5 << 27, (PROBE, 8192, 512, 4, 0, 1, 0)),
    (2_097_929, 100_000, (PROBE, 4096, 98, 8, 0, 1, 0)),
    (1_049_353, 50_000, (PROBE, 4096, 49, 16, 0, 1, 0)),
    (525_065, 20_000, (PROBE, 4096, 20, 32, 0, 1, 0)),
]


# Pass 1's kernel per geometry (bloom_pass1.h choose_pass1_kernel) on a
# 256-CU device, through the micro-benchmark library's ubench_pass1_choice (no
# device call).  Rows: (n keys, m bits, slots: 0 = a build on plan_build, 1 =
# a one-filter partitioned probe on plan_segments, key stride) -> Pass1Kernel's
# fields (super, threads, layout, slots, cols, mk, maxb, workgroups per CU,
# nt, defer, grid).  Every row was worked out by hand from the planners
# (plan_segments, plan_build, choose_tile_keys) and from the launchers as they
# stood before the choice became one function (launch_bin, launch_bin_tb,
# pass1_plan, bin_launch_layout, bin_launch_fast, bin_launch,
# part_bin_wgs_per_cu, launch_bin_super_impl, launch_bin_super_mk), not by
# running choose_pass1_kernel.
PACKED, ENTRY, STRIDED = 0, 1, 2
FAST, WIDE, P2, LADDER, LADDER0, LADDER0R = 0, 1, 2, 3, 4, 5
PASS1_ROWS = [
    # C2 and C5's run: the kernels recorded in profiles/pass1_overlap/
    # kernel_stats_c2_A.csv (k_part_bin<0, false, true, 512, 5, 511, 6, 0,
    # false>: three workgroups per CU, grid 768) and kernel_stats_c5_A.csv
    # (<0, false, true, 1024, 5, 1023, 4, 0, true>, since then also deferred).
    # C5's run table, 8,192 tiles x 512 bins x 4 B, is exactly the 16 MiB of
    # kColumnTableMaxBytes: columns.
    (16_777_216, 167_772_160, 0, 4, (0, 512, PACKED, 0, 1, LADDER0R, 511, 3, 0, 0, 768)),
    (67_108_864, 671_088_640, 0, 4, (0, 1024, PACKED, 0, 1, LADDER0R, 1023, 1, 1, 1, 256)),
    # bin_launch's non-temporal test on C5's geometry: 4,096 tiles of 8192
    # keys are exactly kInfinityCacheBytes (not nt), one key more is nt
    (33_554_432, 671_088_640, 0, 4, (0, 1024, PACKED, 0, 1, LADDER0R, 1023, 1, 0, 1, 256)),
    (33_554_433, 671_088_640, 0, 4, (0, 1024, PACKED, 0, 1, LADDER0R, 1023, 1, 1, 1, 256)),
    # C4 (launch_bin_super_mk): 2,458 segments on 16,384 super-tiles, m =
    # 3 << 30 on segments of 2^18 bits x 5 is kModP2; the run table (161 MB)
    # goes out as rows and is transposed
    (268_435_456, 3 << 30, 0, 4, (1, 1024, PACKED, 0, 0, P2, 4095, 1, 0, 0, 256)),
    # the f = 10 tree's level-2 build: 505 segments (not a p2 form: the general
    # remainder) on 8192-key tiles, 1024 threads, deferred, 128 MiB of tiles
    (16_777_216, 512_000_000, 0, 4, (0, 1024, PACKED, 0, 1, FAST, 1023, 1, 0, 1, 256)),
    # bin_launch_layout's reduction kinds: m = 2^32 is kModWide at the largest
    # capacity (3,277 segments, 123 tiles); m = 100,000,007 the general
    # remainder on 255 segments of 4096-key tiles (245 tiles)
    (1_000_000, 2**32, 0, 4, (0, 1024, PACKED, 0, 1, WIDE, 8192, 1, 0, 1, 123)),
    (1_000_000, 100_000_007, 0, 4, (0, 512, PACKED, 0, 1, FAST, 511, 3, 0, 0, 245)),
    # m = 3 << 26: plan_segments gives 256 segments of 3 << 18 bits, a power of
    # two of them on a p2 form, so plan_build makes it a one-member ladder
    # (s = 18, t = 26: relabelled) and the BUILD is kModLadder0R, not kModP2;
    # the probe of that filter (plan_segments alone) is the kModP2 row below.
    # A build on kModP2 needs p2 segments that are no power of two:
    # m = 51 << 23 (503 segments of 26 << 15 bits).
    (1_000_000, 3 << 26, 0, 4, (0, 512, PACKED, 0, 1, LADDER0R, 511, 3, 0, 0, 245)),
    (1_000_000, 51 << 23, 0, 4, (0, 1024, PACKED, 0, 1, P2, 1023, 1, 0, 1, 123)),
    # key layouts on C2's geometry (bin_launch_layout): entry_t runs keep the
    # small capacity; strided keys take kPartMaxBins and with it two
    # workgroups per CU, not three
    (16_777_216, 167_772_160, 0, 8, (0, 512, ENTRY, 0, 1, LADDER0R, 511, 3, 0, 0, 768)),
    (16_777_216, 167_772_160, 0, 12, (0, 512, STRIDED, 0, 1, LADDER0R, 4096, 2, 0, 0, 512)),
    # bin_launch_fast's capacity steps at 1024 threads, on probes (a build on
    # 1,024-4,095 segments of m < 2^32 sorts super-tiles): 1,023 | 1,024
    # segments (m = 10,230 << 17 and 5 << 28: 10 sub-blocks of 2^17 bits per
    # segment) and 2,047 | 2,048 (m = 10,235 << 18 and 2,684,354,559: 5
    # sub-blocks of 2^18); and 2,048 bins on a build's ladder (m = 5 << 29),
    # deferred and above the nt capacity.  The step 511 | 512 at 512 threads
    # cannot be reached from the planners: choose_tile_keys gives every
    # geometry of more than 256 segments the 8192-key tile, so 512 threads
    # sort at most 256 segments (MAXB 511, or kPartMaxBins for strided keys).
    (1_000_000, 10_230 << 17, 1, 4, (0, 1024, PACKED, 1, 1, FAST, 1023, 1, 0, 0, 123)),
    (1_000_000, 5 << 28, 1, 4, (0, 1024, PACKED, 1, 1, P2, 2047, 1, 0, 0, 123)),
    (1_000_000, 10_235 << 18, 1, 4, (0, 1024, PACKED, 1, 1, FAST, 2047, 1, 0, 0, 123)),
    (1_000_000, 2_684_354_559, 1, 4, (0, 1024, PACKED, 1, 1, FAST, 4095, 1, 0, 0, 123)),
    (1_000_000, 5 << 29, 0, 4, (0, 1024, PACKED, 0, 1, LADDER0R, 4095, 1, 0, 1, 123)),
    # partitioned probes (launch_bin_tb<true, TB>): 256 segments on 4096-key
    # tiles, two workgroups per CU even at MAXB 511 (4,096 tiles: grid 512);
    # C5's filter on 512 segments of 8192-key tiles: 1024 threads and neither
    # deferred nor nt with the slot plane
    (16_777_216, 3 << 26, 1, 4, (0, 512, PACKED, 1, 1, P2, 511, 2, 0, 0, 512)),
    (16_777_216, 671_088_640, 1, 4, (0, 1024, PACKED, 1, 1, P2, 1023, 1, 0, 0, 256)),
    # the single probes of tests/test_gpu_probe_walks.py (PROBE_WALK_ROWS).
    # 5 << 25 (t = 25 >= 21: kModP2) on 256 segments of 4096-key tiles, two
    # 512-thread workgroups per CU: 2C + 1 tiles ending in one key and 2C + 2
    # ending in 4095 keys give a workgroup a second tile (grid 512); entry_t keys
    (2_097_153, 5 << 25, 1, 4, (0, 512, PACKED, 1, 1, P2, 511, 2, 0, 0, 512)),
    (2_105_343, 5 << 25, 1, 4, (0, 512, PACKED, 1, 1, P2, 511, 2, 0, 0, 512)),
    (2_097_929, 5 << 25, 1, 8, (0, 512, ENTRY, 1, 1, P2, 511, 2, 0, 0, 512)),
    # 5 << 27 at 1,025 tiles of 8192 keys; the filters of 98, 49 and 20
    # segments (no p2 form: the general remainder) at 513, 257 and 129 tiles,
    # of which only the first outnumber the 512 resident workgroups
    (8_389_385, 5 << 27, 1, 4, (0, 1024, PACKED, 1, 1, P2, 1023, 1, 0, 0, 256)),
    (2_097_929, 100_000, 1, 4, (0, 512, PACKED, 1, 1, FAST, 511, 2, 0, 0, 512)),
    (1_049_353, 50_000, 1, 4, (0, 512, PACKED, 1, 1, FAST, 511, 2, 0, 0, 257)),
    (525_065, 20_000, 1, 4, (0, 512, PACKED, 1, 1, FAST, 511, 2, 0, 0, 129)),
]


def _pass1_choice(n, m, slots, stride):
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    ub = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    ub.ubench_pass1_choice.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t,
                                       ctypes.c_int, ctypes.c_void_p]
    out = np.zeros(11, dtype=np.int32)
    return ub.ubench_pass1_choice(n, m, slots, stride, 256, out.ctypes.data), tuple(int(x) for x in out)


@pytest.mark.parametrize("n,m,slots,stride,want", PASS1_ROWS)
def test_pass1_kernel_choice(n, m, slots, stride, want):
    assert _pass1_choice(n, m, slots, stride) == (0, want)


def test_pass1_kernel_choice_refusal():
    """m = 2^40 has no segment geometry (a segment of 2^26 bits exceeds the
    LDS image): refused (-34) before a kernel is chosen.  choose_pass1_kernel's
    own refusals (-22: more segments than the family's histogram holds, a
    one-member ladder with slots, a ladder whose bits do not add up to t, a
    super-tile kind other than kModP2 / kModFast) guard against geometries
    plan_build and plan_segments do not produce: they cap the segments per
    tile size, make ladders from p2 forms only and super-tiles for m < 2^32
    only, so none is reachable from here."""
    for slots in (0, 1):
        status, out = _pass1_choice(1_000_000, 1 << 40, slots, 4)
        assert status == -34 and out == (0,) * 11


@pytest.mark.parametrize("n,ms,want", WALK_ROWS)
def test_pass2_walk_choice(n, ms, want):
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    ub = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    ub.ubench_walk_choice.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                      ctypes.c_void_p]
    sizes = np.array(ms, dtype=np.uint64)
    out = np.zeros(7, dtype=np.int32)
    assert ub.ubench_walk_choice(n, len(ms), sizes.ctypes.data, 256, out.ctypes.data) == 0
    assert tuple(int(x) for x in out) == want


def _probe_walk_choice(n, m):
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    ub = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    ub.ubench_probe_walk_choice.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    out = np.zeros(7, dtype=np.int32)
    return ub.ubench_probe_walk_choice(n, m, 256, out.ctypes.data), tuple(int(x) for x in out)


@pytest.mark.parametrize("n,m,want", PROBE_WALK_ROWS)
def test_probe_walk_choice(n, m, want):
    assert _probe_walk_choice(n, m) == (0, want)


def test_probe_walk_choice_refusal():
    """m = 2^40 has no segment geometry (test_pass1_kernel_choice_refusal)."""
    assert _probe_walk_choice(1_000_000, 1 << 40) == (-34, (0,) * 7)


# ---------------------------------------------------------------------------
# The run table's layout (bloom_kernels.hip runs_as_columns): columns while
# ntiles * nbins * 4 <= kColumnTableMaxBytes (16 MiB), rows and the transpose
# above; BLOOMHIP_RUN_TABLE = rows | cols forces one, read on every call.
# ---------------------------------------------------------------------------
def _with_cols(want, cols):
    return want[:4] + (cols,) + want[5:]


def test_run_table_variable_forces_the_layout(monkeypatch):
    """rows turns C2's columns into rows, cols turns C4's rows into columns;
    no other field of the choice moves."""
    c2, c4 = PASS1_ROWS[0], PASS1_ROWS[4]
    assert c2[:2] == (16_777_216, 167_772_160) and c2[4][4] == 1
    assert c4[:2] == (268_435_456, 3 << 30) and c4[4][4] == 0
    monkeypatch.setenv("BLOOMHIP_RUN_TABLE", "rows")
    assert _pass1_choice(*c2[:4]) == (0, _with_cols(c2[4], 0))
    assert _pass1_choice(*c4[:4]) == (0, c4[4])
    monkeypatch.setenv("BLOOMHIP_RUN_TABLE", "cols")
    assert _pass1_choice(*c4[:4]) == (0, _with_cols(c4[4], 1))
    assert _pass1_choice(*c2[:4]) == (0, c2[4])
    monkeypatch.delenv("BLOOMHIP_RUN_TABLE")
    assert _pass1_choice(*c2[:4]) == (0, c2[4])
    assert _pass1_choice(*c4[:4]) == (0, c4[4])


@pytest.mark.parametrize("value", [None, "", "columns", "ROWS", "row", "cols ", "0"])
def test_run_table_variable_unset_or_junk_keeps_the_rule(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("BLOOMHIP_RUN_TABLE", raising=False)
    else:
        monkeypatch.setenv("BLOOMHIP_RUN_TABLE", value)
    for n, m, slots, stride, want in PASS1_ROWS:
        assert _pass1_choice(n, m, slots, stride) == (0, want), (n, m, slots, stride)


# Both sides of the threshold on a 256-CU device, per family.  The table is
# columns while ntiles * segments <= 2^24 / 4, so the most tiles that still
# give columns are 2^22 // segments, and rows start one key past that many
# full tiles.  Segments and tile keys are the planners' (WALK_ROWS and the
# comments of PASS1_ROWS; m = 2^33 - 7: plan_segments takes s = 19 (16,384
# sub-blocks), 26 rounds of 256 CUs want 6,656 segments, g = 3 sub-blocks
# exceed the 160 KiB image, so g = 2: 8,192 segments of 2^20 bits, 8192-key
# tiles as m > 2^32 - 1 sorts no super-tiles), worked out by hand:
#   8,192 segments: 2^22 // 8192 =    512 tiles x  8192 + 1 =  4,194,305
#   3,277 segments: 2^22 // 3277 =  1,279 tiles x  8192 + 1 = 10,477,569
#   3,277 segments on super-tiles:  1,279     x 16,384 + 1 = 20,955,137
#     256 segments: 2^22 //  256 = 16,384 tiles x  4096 + 1 = 67,108,865
#     255 segments: 2^22 //  255 = 16,448 tiles x  4096 + 1 = 67,371,009
#     512 segments: 2^22 //  512 =  8,192 tiles x  8192 + 1 = 67,108,865
# Rows: (m, slots, segments, tile keys, first n with rows, the choice there).
RUN_TABLE_THRESHOLDS = [
    (2**33 - 7, 0, 8192, 8192, 4_194_305, (0, 1024, PACKED, 0, 0, WIDE, 8192, 1, 0, 1, 256)),
    (2**32, 0, 3277, 8192, 10_477_569, (0, 1024, PACKED, 0, 0, WIDE, 8192, 1, 0, 1, 256)),
    (2**32 - 1, 0, 3277, 16_384, 20_955_137, (1, 1024, PACKED, 0, 0, FAST, 4095, 1, 0, 0, 256)),
    # C2's filter: the pipelined 512-thread kernel (ubench_pass1_pipe below)
    (5 << 25, 0, 256, 4096, 67_108_865, (0, 512, PACKED, 0, 0, LADDER0R, 511, 3, 0, 0, 768)),
    (100_000_007, 0, 255, 4096, 67_371_009, (0, 512, PACKED, 0, 0, FAST, 511, 3, 0, 0, 768)),
    # C5's filter: deferred and non-temporal
    (5 << 27, 0, 512, 8192, 67_108_865, (0, 1024, PACKED, 0, 0, LADDER0R, 1023, 1, 1, 1, 256)),
    # the one-filter partitioned probe of m = 2^33 - 7
    (2**33 - 7, 1, 8192, 8192, 4_194_305, (0, 1024, PACKED, 1, 0, WIDE, 8192, 1, 0, 0, 256)),
]


@pytest.mark.parametrize("m,slots,segments,tile,n_rows,want", RUN_TABLE_THRESHOLDS)
def test_run_table_threshold_both_sides(monkeypatch, m, slots, segments, tile, n_rows, want):
    monkeypatch.delenv("BLOOMHIP_RUN_TABLE", raising=False)
    most_column_tiles = (16 << 20) // 4 // segments
    assert most_column_tiles * segments * 4 <= 16 << 20 < (most_column_tiles + 1) * segments * 4
    assert n_rows == most_column_tiles * tile + 1
    assert _pass1_choice(n_rows, m, slots, 4) == (0, want)
    assert _pass1_choice(n_rows - 1, m, slots, 4) == (0, _with_cols(want, 1))


def test_run_table_threshold_pipelined_family(monkeypatch):
    """The 512-thread build of 5 << 25 past the threshold is the pipelined kernel."""
    monkeypatch.delenv("BLOOMHIP_RUN_TABLE", raising=False)
    ub = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    ub.ubench_pass1_pipe.argtypes = [ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t,
                                     ctypes.c_int, ctypes.c_void_p]
    out = ctypes.c_int(-1)
    assert ub.ubench_pass1_pipe(67_108_865, 5 << 25, 0, 4, 256, ctypes.byref(out)) == 0
    assert out.value == 1


def _stack_pass1_choice(n, ms, stride=4, cu_count=256):
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    ub = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    ub.ubench_stack_pass1_choice.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    sizes = np.array(ms, dtype=np.uint64)
    out = np.zeros(11, dtype=np.int32)
    rc = ub.ubench_stack_pass1_choice(n, len(ms), sizes.ctypes.data, stride, cu_count, out.ctypes.data)
    return rc, tuple(int(x) for x in out)


def test_stack_pass1_kernel_choice(monkeypatch):
    """Pass 1 of a stacked probe through ubench_stack_pass1_choice, 16.8M GETs
    on 256 CUs.  The f = 10 tree's three levels: WALK_ROWS' segment stack on
    1,250 segments of 16,384-key super-tiles, so k_part_bin2 with the slot
    plane (launch_pass1_super: 1024 threads, the one capacity kSuperMaxBins,
    one workgroup per CU, 1,024 tiles on 256 persistent workgroups); m_max =
    512,000,000 = 15,625 << 15 is no p2 form: the general remainder.  C3's
    five levels: WALK_ROWS' ladder on 256 bins of 8192-key tiles, so the
    1024-thread k_part_bin with slots on kModLadder at MAXB 1023, neither
    deferred nor non-temporal with the slot plane.  Both tables (1,024 x
    1,250 and 2,048 x 256 words) are columns."""
    monkeypatch.delenv("BLOOMHIP_RUN_TABLE", raising=False)
    f10 = [5_120_000 * 10**i for i in range(3)]
    c3 = [655_360 * 4**i for i in range(4, -1, -1)]
    walk = {tuple(ms): want for _, ms, want in WALK_ROWS}
    assert walk[tuple(f10[::-1])][:3] == (STACK, 16_384, 1250)
    assert walk[tuple(c3)][:3] == (LADDER, 8192, 256)
    want_f10 = (1, 1024, PACKED, 1, 1, FAST, 4095, 1, 0, 0, 256)
    assert _stack_pass1_choice(16_777_216, f10) == (0, want_f10)
    assert _stack_pass1_choice(16_777_216, f10[::-1]) == (0, want_f10)
    want_c3 = (0, 1024, PACKED, 1, 1, 3, 1023, 1, 0, 0, 256)  # mk 3: kModLadder
    assert _stack_pass1_choice(16_777_216, c3) == (0, want_c3)
    # entry_t keys, and the variable through this export as well
    assert _stack_pass1_choice(16_777_216, c3, stride=8) == (0, want_c3[:2] + (ENTRY,) + want_c3[3:])
    monkeypatch.setenv("BLOOMHIP_RUN_TABLE", "rows")
    assert _stack_pass1_choice(16_777_216, f10) == (0, _with_cols(want_f10, 0))
    assert _stack_pass1_choice(16_777_216, c3) == (0, _with_cols(want_c3, 0))
    # one filter is no stack; sizes with no common segment width have no geometry
    assert _stack_pass1_choice(1000, [5 << 25])[0] == -22
    assert _stack_pass1_choice(1000, [1_000_000, 1_000_000])[0] == -34


# Pass 1 of the stacked probes of tests/test_gpu_probe_walks.py on 256 CUs, at
# their 513-tile shapes (WALK_ROWS has the segments and tile keys of each).
# Rows: (n, member sizes, key stride) -> Pass1Kernel's fields as in PASS1_ROWS.
# The f = 10 tree on super-tiles: one workgroup per CU, so 513 tiles are a
# second and a third tile for workgroup 0; 625 segments: MAXB 1023; 6,144
# segments of 3 << 26 (t = 26: kModP2): only the full capacity 8192 holds them;
# 256 and 100 segments on 4096-key tiles: 512 threads, MAXB 511, two workgroups
# per CU with the slot plane (3 << 20 has t = 20 < 21: the general remainder,
# as 12,800 = 25 << 9); C3's ladder on 8192-key tiles (kModLadder = 3).
STACK_PASS1_ROWS = [
    (8_389_385, [512_000_000, 51_200_000, 5_120_000], 4, (1, 1024, PACKED, 1, 1, FAST, 4095, 1, 0, 0, 256)),
    (4_195_081, [512_000_000, 51_200_000, 5_120_000], 8, (1, 1024, ENTRY, 1, 1, FAST, 4095, 1, 0, 0, 256)),
    (4_195_081, [256_000_000, 25_600_000, 2_560_000], 4, (0, 1024, PACKED, 1, 1, FAST, 1023, 1, 0, 0, 256)),
    (4_195_081, [3 << 26, 1 << 15], 4, (0, 1024, PACKED, 1, 1, P2, 8192, 1, 0, 0, 256)),
    (2_097_929, [3 << 20, 1 << 20, 3 << 18, 1 << 18, 1 << 19, 3 << 17, 1 << 17, 1 << 16], 4,
     (0, 512, PACKED, 1, 1, FAST, 511, 2, 0, 0, 512)),
    (2_097_929, [12_800, 6_400, 3_200], 4, (0, 512, PACKED, 1, 1, FAST, 511, 2, 0, 0, 512)),
    (4_195_081, [655_360 * 4 ** i for i in range(4, -1, -1)], 4, (0, 1024, PACKED, 1, 1, 3, 1023, 1, 0, 0, 256)),
    (2_097_929, [655_360 * 4 ** i for i in range(4, -1, -1)], 8, (0, 1024, ENTRY, 1, 1, 3, 1023, 1, 0, 0, 256)),
]


@pytest.mark.parametrize("n,ms,stride,want", STACK_PASS1_ROWS)
def test_stack_pass1_kernel_choice_probe_walk_shapes(monkeypatch, n, ms, stride, want):
    monkeypatch.delenv("BLOOMHIP_RUN_TABLE", raising=False)
    assert _stack_pass1_choice(n, ms, stride=stride) == (0, want)
