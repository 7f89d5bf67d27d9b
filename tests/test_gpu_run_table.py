"""Pass 1's tile-major run table and its transpose (k_part_bin / k_part_bin2
with COLS = false, k_runs_transpose).  Pass 1 writes one packed run per (tile,
segment): straight into the segment-major table pass 2 reads while that table
is at most 16 MiB, else into a tile-major table that k_runs_transpose turns
into the segment-major one (bloom_kernels.hip runs_as_columns).  At the sizes
the rest of the suite uses, only C4 takes the second form.  Here:

  (a) the product's transpose alone, against numpy's, at tile counts and
      widths around its 64 x 64 block, with guard words around the output;
  (b) every pass-1 family with the rows layout forced (BLOOMHIP_RUN_TABLE =
      rows) at the smallest shapes its tile loop can go wrong at, and at 63,
      64 and 65 tiles, each with a short last tile; one build and one stack
      with columns forced;
  (c) the 16 MiB rule itself, variable unset, at the smallest batches that
      cross it.

Builds and probes are bit-exact against the C oracle.  No case is vacuous:
each first asks the host choice (ubench_pass1_choice, ubench_stack_pass1_choice
at the device's CU count) for its geometry's layout, and then reads from the
profile slots that the partitioned path ran, once, and nothing else did.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import bloomhip as bh
from bloom_oracle import unpack_bools
from test_gpu_parity import SUPER_MS, _stack_case, rand_keys
from test_gpu_pass1_pipeline import (counts_4096, counts_8192, cu_count, keys_of, partition_build,
                                     want_build)
from test_gpu_pass1_scatter_overlap import count_of, pipe_of

pytestmark = pytest.mark.gpu

# Pass1Kernel's fields as ubench_pass1_choice returns them, and the kinds
SUPER, THREADS, LAYOUT, SLOTS, COLS, MK, MAXB = range(7)
FAST, WIDE, P2, LADDER, LADDER0, LADDER0R = range(6)
STACK_MODE, LADDER_MODE = 2, 3   # ubench_walk_choice's mode of a stacked probe
TABLE_WORDS = (16 << 20) // 4    # kColumnTableMaxBytes in run-table cells
MT = min(16, os.cpu_count() or 1)


@functools.lru_cache(maxsize=None)
def ub():
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    L = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    SZ, I, P = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    L.ubench_pass1_choice.argtypes = [SZ, ctypes.c_uint64, I, SZ, I, P]
    L.ubench_stack_pass1_choice.argtypes = [SZ, I, P, SZ, I, P]
    L.ubench_walk_choice.argtypes = [SZ, I, P, I, P]
    L.ubench_runs_transpose.argtypes = [P, P, SZ, I, P]
    return L


def pass1_choice(n, m, slots, stride=4):
    out = np.zeros(11, dtype=np.int32)
    assert ub().ubench_pass1_choice(n, m, slots, stride, cu_count(), out.ctypes.data) == 0
    return tuple(int(x) for x in out)


def stack_pass1_choice(n, ms, stride=4):
    sizes = np.array(sorted(ms, reverse=True), dtype=np.uint64)  # largest first, as the product sorts
    out = np.zeros(11, dtype=np.int32)
    assert ub().ubench_stack_pass1_choice(n, len(ms), sizes.ctypes.data, stride, cu_count(),
                                          out.ctypes.data) == 0
    return tuple(int(x) for x in out)


def walk_choice(n, ms):
    """(mode, tile keys, segments) of a build (one size) or a stacked probe."""
    sizes = np.array(sorted(ms, reverse=True), dtype=np.uint64)
    out = np.zeros(7, dtype=np.int32)
    assert ub().ubench_walk_choice(n, len(ms), sizes.ctypes.data, cu_count(), out.ctypes.data) == 0
    return tuple(int(x) for x in out[:3])


@pytest.fixture
def ran(monkeypatch):
    """Every set_batch and test_batch of the test runs profiled; ran["set"] and
    ran["test"] list each call's profile slots as {slot: launches}."""
    log = {"set": [], "test": []}
    real_set, real_test = bh.BloomFilter.set_batch, bh.test_batch

    def profiled(f, kind, call):
        f.profile(True)
        f.profile_reset()
        try:
            out = call()
            log[kind].append({k: v["launches"] for k, v in f.profile_read().items()})
        finally:
            f.profile(False)
        return out

    def set_batch(self, *a, **kw):
        return profiled(self, "set", lambda: real_set(self, *a, **kw))

    def test_batch(filters, *a, **kw):
        return profiled(filters[0], "test", lambda: real_test(filters, *a, **kw))

    monkeypatch.setattr(bh.BloomFilter, "set_batch", set_batch)
    monkeypatch.setattr(bh, "test_batch", test_batch)
    return log


def partitioned_build_ran(slots):
    return (slots.get("k_part_bin") == 1 and slots.get("k_part_apply") == 1 and
            "k_build_atomic" not in slots and "k_build_lds" not in slots)


def partitioned_probe_ran(slots, which):
    others = {"k_probe", "k_probe_lds", "probe_partitioned", "probe_stacked"} - {which}
    return slots.get(which) == 1 and not others & set(slots)


def want_bitmap(coracle, m, n):
    """The oracle's bitmap for keys_of(n): cached below 2^31 bits (shared with
    the tile-loop tests), rebuilt per case above (256 MiB and more each)."""
    return want_build(coracle, m, n) if m < 2**31 else coracle.build(m, keys_of(n))


def checked_build(coracle, ran, m, n, cols, stride=4):
    """A partition build of keys_of(n) at `stride`, bit-exact against the
    oracle, after the host choice for it gave the layout `cols`; the choice."""
    choice = pass1_choice(n, m, 0, stride)
    assert choice[COLS] == cols and choice[SLOTS] == 0
    if stride == 4:
        f = partition_build(m, keys_of(n))
    else:
        aos = np.zeros((n, stride // 4), dtype=np.int32)
        aos[:, 0] = keys_of(n)
        f = partition_build(m, aos.reshape(-1), n=n, stride=stride)
    assert partitioned_build_ran(ran["set"][-1]), ran["set"][-1]
    assert (f.words() == want_bitmap(coracle, m, n)).all()
    return f, choice


# --------------------------------------------------- (a) the transpose ----
SENTINEL = 0xDEADBEEF
GUARD = 64 * 65 + 31   # words either side of the output, past one 64 x 64 block


@pytest.mark.parametrize("width", [1, 20, 63, 64, 65, 255, 256, 505, 2458, 8192])
@pytest.mark.parametrize("ntiles", [1, 2, 63, 64, 65, 128, 129, 1281])
def test_product_transpose_matches_numpy(ntiles, width):
    """k_runs_transpose through launch_runs_transpose: blocks whose clamped
    loads and guarded stores cut off in tiles, in segments, and in both."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rng = np.random.default_rng(ntiles * 10_007 + width)
    rows = rng.integers(0, 2**32, size=(ntiles, width), dtype=np.uint64).astype(np.uint32)
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    cells = ntiles * width
    d_out = torch.from_numpy(np.full(GUARD + cells + GUARD, SENTINEL, dtype=np.uint32).view(np.int32)).cuda()
    assert ub().ubench_runs_transpose(d_rows.data_ptr(), d_out.data_ptr() + 4 * GUARD, ntiles, width,
                                      None) == 0
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[:GUARD] == SENTINEL).all() and (out[GUARD + cells:] == SENTINEL).all()
    assert (out[GUARD:GUARD + cells].reshape(width, ntiles) == rows.T).all()


# -------------------------------------- (b) rows forced, smallest shapes ----
@pytest.fixture
def rows(monkeypatch):
    monkeypatch.setenv("BLOOMHIP_RUN_TABLE", "rows")


def shapes_4096():
    c = counts_4096()
    return {
        "only_short": c["only_short"], "full_into_short": c["full_into_short"],
        "three_rounds": c["three_rounds"], "four_rounds": count_of("four_rounds"),
        # around the transpose's 64-tile block, each with a short last tile
        "tiles63": 62 * 4096 + 5, "tiles64": 63 * 4096 + 4095, "tiles65": 64 * 4096 + 1,
    }


# the 512-thread builds: the reduction kind and the tile loop of each filter
# (tests/test_host.py PASS1_ROWS; m = 100,000: 98 segments, pass 2's batch walk)
BUILDS_512 = {5 << 25: (LADDER0R, 1), 3 << 26: (LADDER0R, 1), 100_000_007: (FAST, 0), 100_000: (FAST, 0)}


@pytest.mark.parametrize("shape", ["only_short", "full_into_short", "three_rounds", "four_rounds",
                                   "tiles63", "tiles64", "tiles65"])
@pytest.mark.parametrize("m", list(BUILDS_512), ids=["ladder_pipelined", "p2_pipelined", "general", "batch_walk"])
def test_rows_build_512_threads(coracle, ran, rows, m, shape):
    n = shapes_4096()[shape]
    mk, pipe = BUILDS_512[m]
    _, choice = checked_build(coracle, ran, m, n, cols=0)
    assert (choice[SUPER], choice[THREADS], choice[MK]) == (0, 512, mk)
    assert pipe_of(n, m, 4) == pipe


@pytest.mark.parametrize("stride", [8, 12])
@pytest.mark.parametrize("m", [5 << 25, 100_000_007], ids=["ladder_pipelined", "general"])
def test_rows_build_512_threads_key_layouts(coracle, ran, rows, m, stride):
    """entry_t keys (the pipelined loop on the ladder) and 12-byte records
    (two workgroups per CU at the largest capacity, the plain loop)."""
    n = shapes_4096()["full_into_short"]
    _, choice = checked_build(coracle, ran, m, n, cols=0, stride=stride)
    assert (choice[THREADS], choice[LAYOUT]) == (512, 1 if stride == 8 else 2)


def test_rows_build_512_threads_merges_second_batch(coracle, ran, rows):
    """A second batch ORed into the built filter: pass 2's merging write-back
    reads the transposed table too."""
    m, n = 5 << 25, shapes_4096()["full_into_short"]
    f, _ = checked_build(coracle, ran, m, n, cols=0)
    more = keys_of(n, seed=1)
    f.set_batch(more)
    assert partitioned_build_ran(ran["set"][-1]), ran["set"][-1]
    want = want_build(coracle, m, n).copy()
    coracle.set_into(want, m, more)
    assert (f.words() == want).all()


def shapes_8192():
    c = counts_8192()
    return {"only_short": c["only_short"], "full_into_short": c["full_into_short"],
            "tiles65": 64 * 8192 + 77}


# the 1024-thread builds: (kind, capacity) per filter
BUILDS_1024 = {5 << 27: (LADDER0R, 1023), 512_000_000: (FAST, 1023), 51 << 23: (P2, 1023),
               2**32: (WIDE, 8192), 5 << 29: (LADDER0R, 4095)}


@pytest.mark.parametrize("shape", ["only_short", "full_into_short", "tiles65"])
@pytest.mark.parametrize("m", list(BUILDS_1024), ids=["ladder", "general", "p2", "wide", "ladder_2048_bins"])
def test_rows_build_1024_threads(coracle, ran, rows, m, shape):
    n = shapes_8192()[shape]
    _, choice = checked_build(coracle, ran, m, n, cols=0)
    assert (choice[SUPER], choice[THREADS], choice[MK], choice[MAXB]) == (0, 1024) + BUILDS_1024[m]


@pytest.mark.parametrize("stride", [8, 12])
def test_rows_build_1024_threads_key_layouts(coracle, ran, rows, stride):
    n = shapes_8192()["full_into_short"]
    _, choice = checked_build(coracle, ran, 5 << 27, n, cols=0, stride=stride)
    assert (choice[THREADS], choice[LAYOUT]) == (1024, 1 if stride == 8 else 2)


@pytest.mark.parametrize("n", [1, 16_385, 65 * 16_384 + 3])
@pytest.mark.parametrize("m", SUPER_MS)
def test_rows_build_super_tiles(coracle, ran, rows, m, n):
    _, choice = checked_build(coracle, ran, m, n, cols=0)
    assert (choice[SUPER], choice[THREADS]) == (1, 1024)


def test_rows_build_super_tiles_entry_keys(coracle, ran, rows):
    _, choice = checked_build(coracle, ran, SUPER_MS[1], 65 * 16_384 + 3, cols=0, stride=8)
    assert (choice[SUPER], choice[LAYOUT]) == (1, 1)


def checked_probe(coracle, ran, m, n, cols, mt=1):
    """A one-filter partitioned probe of n keys against a filter of 40,000,
    some of them planted at both ends of the batch; the host choice."""
    choice = pass1_choice(n, m, 1)
    assert choice[COLS] == cols and choice[SLOTS] == 1
    members = keys_of(40_000, seed=2)
    f = bh.BloomFilter(m)
    f.set_probe_strategy(bh.PROBE_PARTITION)
    f.set_batch(members)
    probe = rand_keys(n, seed=3)
    probe[:5000] = members[:5000]
    probe[n - 5000:] = members[5000:10_000]
    got = bh.test_batch([f], probe)[0]
    assert partitioned_probe_ran(ran["test"][-1], "probe_partitioned"), ran["test"][-1]
    ref = coracle.build(m, members)
    want = coracle.test(ref, m, probe) if mt == 1 else coracle.test_mt(ref, m, probe, mt)
    assert (got == want).all()
    hits = unpack_bools(got, n)
    assert hits[:5000].all() and hits[n - 5000:].all()
    return choice


# one-filter partitioned probes: (threads, kind, capacity) per filter
PROBES = {3 << 26: (512, P2, 511), 671_088_640: (1024, P2, 1023), 10_230 << 17: (1024, FAST, 1023),
          2_684_354_559: (1024, FAST, 4095), 2**32 + 15: (1024, WIDE, 8192)}


@pytest.mark.parametrize("m", list(PROBES), ids=["512_threads", "c5_filter", "1023_segments",
                                                  "2048_segments", "wide"])
def test_rows_partitioned_probe(coracle, ran, rows, m):
    threads = PROBES[m][0]
    choice = checked_probe(coracle, ran, m, 65 * threads * 8 + 1, cols=0)
    assert (choice[SUPER], choice[THREADS], choice[MK], choice[MAXB]) == (0,) + PROBES[m]


# stacked probes: (sizes, pass 2's mode, tile keys, pass 1 on super-tiles)
STACKS = {
    "c3_ladder": ([655_360 * 4**i for i in range(5)], LADDER_MODE, 8192, 0),
    "segments": ([3 * 2**20, 2**20, 3 * 2**18, 2**18], STACK_MODE, 4096, 0),
    "f10_super_tiles": ([5_120_000 * 10**i for i in range(3)], STACK_MODE, 16_384, 1),
}


def checked_stack(coracle, ran, which, tiles, cols, stride=4):
    ms, mode, tile, super_tiles = STACKS[which]
    n = tiles * tile + 1
    assert walk_choice(n, ms)[:2] == (mode, tile)
    choice = stack_pass1_choice(n, ms, stride)
    assert (choice[SUPER], choice[THREADS], choice[SLOTS], choice[COLS]) == \
        (super_tiles, 512 if tile == 4096 else 1024, 1, cols)
    _stack_case(coracle, ms, rand_keys(n, seed=60 + tiles), stride=stride, seed=20 + tiles)
    assert partitioned_probe_ran(ran["test"][-1], "probe_stacked"), ran["test"][-1]


@pytest.mark.parametrize("tiles", [0, 1, 65], ids=["one_key", "tile_plus_1", "65_tiles_plus_1"])
@pytest.mark.parametrize("which", list(STACKS))
def test_rows_stacked_probe(coracle, ran, rows, which, tiles):
    checked_stack(coracle, ran, which, tiles, cols=0)


@pytest.mark.parametrize("which", list(STACKS))
def test_rows_stacked_probe_entry_keys(coracle, ran, rows, which):
    checked_stack(coracle, ran, which, 1, cols=0, stride=8)


def test_forced_columns_build_and_stack(coracle, ran, monkeypatch):
    """The variable's other value through the whole path."""
    monkeypatch.setenv("BLOOMHIP_RUN_TABLE", "cols")
    checked_build(coracle, ran, 5 << 25, shapes_4096()["tiles65"], cols=1)
    checked_stack(coracle, ran, "f10_super_tiles", 1, cols=1)


# ------------------------------------ (c) the rule, the variable unset ----
@pytest.fixture
def rule(monkeypatch):
    monkeypatch.delenv("BLOOMHIP_RUN_TABLE", raising=False)


def first_rows_n(m, slots):
    """The smallest n whose run table exceeds 16 MiB, from the device's
    geometry: one key past the most full tiles that still give columns; the
    layout is checked on both sides, at n and one tile below."""
    _, tile, segments = walk_choice(1, [m])
    n = TABLE_WORDS // segments * tile + 1
    assert pass1_choice(n, m, slots)[COLS] == 0
    assert pass1_choice(n - tile, m, slots)[COLS] == 1
    return n


def big_build(coracle, ran, m, n, cols, seed):
    choice = pass1_choice(n, m, 0)
    assert choice[COLS] == cols
    keys = rand_keys(n, seed)
    f = partition_build(m, keys)
    assert partitioned_build_ran(ran["set"][-1]), ran["set"][-1]
    assert (f.words() == coracle.build_mt(m, keys, MT)).all()
    return choice


@pytest.mark.parametrize("side", ["rows", "last_columns"])
def test_rule_build_wide(coracle, ran, rule, side):
    """m = 2^33 - 7 (8,192 segments, kModWide): rows from about 4.2M keys; the
    largest batch that still gives columns builds the same way."""
    m = 2**33 - 7
    n = first_rows_n(m, 0)
    assert 4_000_000 < n < 4_400_000
    choice = big_build(coracle, ran, m, n if side == "rows" else n - 1, 0 if side == "rows" else 1, 71)
    assert (choice[THREADS], choice[MK]) == (1024, WIDE)


def test_rule_partitioned_probe_wide(coracle, ran, rule):
    m = 2**33 - 7
    n = first_rows_n(m, 1)
    assert 4_000_000 < n < 4_400_000
    choice = checked_probe(coracle, ran, m, n, cols=0, mt=MT)
    assert (choice[THREADS], choice[MK]) == (1024, WIDE)


def test_rule_build_super_tiles(coracle, ran, rule):
    m = 2**32 - 1
    n = first_rows_n(m, 0)
    assert 20_000_000 < n < 22_000_000
    choice = big_build(coracle, ran, m, n, 0, 72)
    assert (choice[SUPER], choice[MK]) == (1, FAST)


def test_rule_build_pipelined(coracle, ran, rule):
    """The smallest batch that gives the pipelined 512-thread family (C2's
    filter, 256 bins of 4096-key tiles) a row table: 16,385 tiles."""
    m = 5 << 25
    n = first_rows_n(m, 0)
    assert 67_000_000 < n < 67_200_000
    assert pipe_of(n, m, 4) == 1
    choice = big_build(coracle, ran, m, n, 0, 73)
    assert (choice[SUPER], choice[THREADS], choice[MK]) == (0, 512, LADDER0R)
