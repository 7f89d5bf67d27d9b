"""Pass 1's tile loop and write-out (k_part_bin).  In the 1024-thread builds
a sorted tile goes out during the hash phase of its workgroup's next tile and
the block's last tile in an epilogue; the other families write a tile out
after its own scatter.  Both loops are walked here through every shape of a
block's rounds: only a short tile, one full tile, a full tile followed by a
1-key or a short tile, three rounds.

The shapes are the smallest at which that can go wrong, placed by the device's
CU count C: a workgroup's rounds are decided by the tile count against the
grid (three 512-thread workgroups per CU on 4096-key build tiles, one
1024-thread workgroup per CU on 8192-key tiles).  Everything is compared
bit-exactly with the C oracle, on the partition paths explicitly.
"""
import functools

import numpy as np
import pytest

import bloomhip as bh

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def cu_count():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def keys_of(n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    k = rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
    k[:min(n, 6)] = [0, -1, 1, 2**31 - 1, -2**31, 13141][:min(n, 6)]
    k.setflags(write=False)
    return k


_WANT = {}


def want_build(coracle, m, n):
    """The oracle's bitmap for keys_of(n), computed once per (m, n)."""
    if (m, n) not in _WANT:
        w = coracle.build(m, keys_of(n))
        w.setflags(write=False)
        _WANT[(m, n)] = w
    return _WANT[(m, n)]


def partition_build(m, keys, **kw):
    f = bh.BloomFilter(m)
    f.set_strategy(bh.BUILD_PARTITION)
    f.set_batch(keys, **kw)
    return f


# 4096-key tiles on G = 3C workgroups: the loop that writes a tile out after its scatter
def counts_4096():
    g = 3 * cu_count()
    return {
        "only_short": 65_549,                    # a block whose only tile is the short one
        "one_full_each": 4096 * g,               # every block exactly one full tile
        "full_into_1key": 4096 * g + 1,          # a full tile, then a 1-key tile
        "full_into_short": 4096 * (g + 1) + 4095,  # a full tile, then the short tile
        "three_rounds": 4096 * (2 * g + 5) + 17,   # a third round for a few blocks
    }


CASES_4096 = ["only_short", "one_full_each", "full_into_1key", "full_into_short", "three_rounds"]


@pytest.mark.parametrize("case", CASES_4096)
@pytest.mark.parametrize("m", [5 << 25, 3 << 26, 100_000_007], ids=["ladder", "p2", "general"])
def test_build_rounds_match_oracle(coracle, m, case):
    n = counts_4096()[case]
    f = partition_build(m, keys_of(n))
    assert (f.words() == want_build(coracle, m, n)).all()


# 8192-key tiles on C workgroups of 1024 threads: the loop that defers
def counts_8192():
    c = cu_count()
    return {
        "only_short": 5_003,                       # a block whose only tile is the short one
        "one_key_tail": 8192 * c + 1,              # a full tile deferred into a 1-key tile
        "full_into_short": 8192 * (c + 1) + 8191,  # full into full + epilogue; full into short
        "three_rounds": 8192 * (2 * c + 5) + 17,   # a deferring tile's own write-out deferred
    }


M_8192 = 5 << 27


@pytest.mark.parametrize("which", ["only_short", "one_key_tail", "full_into_short", "three_rounds"])
def test_build_8192_key_tiles_match_oracle(coracle, which):
    n = counts_8192()[which]
    f = partition_build(M_8192, keys_of(n))
    assert (f.words() == want_build(coracle, M_8192, n)).all()


@pytest.mark.parametrize("stride", [8, 12])
def test_build_8192_key_tiles_key_layouts(coracle, stride):
    """The deferring loop's entry_t (stride 8) and strided (12-byte) instantiations."""
    n = counts_8192()["full_into_short"]
    aos = np.zeros((n, stride // 4), dtype=np.int32)
    aos[:, 0] = keys_of(n)
    f = partition_build(M_8192, aos.reshape(-1), n=n, stride=stride)
    assert (f.words() == want_build(coracle, M_8192, n)).all()


@pytest.mark.parametrize("stride", [8, 12])
def test_build_key_layouts_match_oracle(coracle, stride):
    """entry_t keys (stride 8, 16-B aligned) and 12-byte records."""
    n = counts_4096()["full_into_short"]
    m = 5 << 25
    keys = keys_of(n)
    aos = np.zeros((n, stride // 4), dtype=np.int32)
    aos[:, 0] = keys
    f = partition_build(m, aos.reshape(-1), n=n, stride=stride)
    assert (f.words() == want_build(coracle, m, n)).all()


def test_build_merges_second_batch(coracle):
    """A second batch of the same count ORed into a built filter."""
    n = counts_4096()["full_into_short"]
    m = 5 << 25
    more = keys_of(n, seed=1)
    f = partition_build(m, keys_of(n))
    f.set_batch(more)
    want = want_build(coracle, m, n).copy()
    coracle.set_into(want, m, more)
    assert (f.words() == want).all()


# ---------------------------------------------------------------- probe ----
def probe_counts():
    c = cu_count()
    return {"one_key_tail": 8192 * c + 1, "full_into_short": 8192 * (c + 1) + 8191}


@pytest.mark.parametrize("which", ["one_key_tail", "full_into_short"])
def test_partitioned_probe_matches_oracle(coracle, which):
    n = probe_counts()[which]
    m = 5 << 25
    members = keys_of(200_000, seed=2)
    f = bh.BloomFilter(m)
    f.set_probe_strategy(bh.PROBE_PARTITION)
    f.set_batch(members)
    probe = keys_of(n, seed=3).copy()
    probe[-50_000:] = members[:50_000]   # hits in the last tiles too
    probe[:50_000] = members[50_000:100_000]
    got = bh.test_batch([f], probe)[0]
    assert (got == coracle.test(coracle.build(m, members), m, probe)).all()


@pytest.mark.parametrize("which", ["one_key_tail", "full_into_short"])
def test_ladder_stack_probe_matches_oracle(coracle, which):
    n = probe_counts()[which]
    ms = [655_360 * 4**i for i in range(3)]
    probe = keys_of(n, seed=4).copy()
    filters, refs = [], []
    for j, m in enumerate(ms):
        members = keys_of(40_000, seed=10 + j)
        f = bh.BloomFilter(m)
        f.set_probe_strategy(bh.PROBE_STACKED)
        f.set_batch(members)
        filters.append(f)
        refs.append((m, coracle.build(m, members)))
        probe[j * 1000:(j + 1) * 1000] = members[:1000]
        probe[n - (j + 1) * 1000:n - j * 1000] = members[1000:2000]
    got = bh.test_batch(filters, probe)
    for j, (m, w) in enumerate(refs):
        assert (got[j] == coracle.test(w, m, probe)).all(), (j, m)
