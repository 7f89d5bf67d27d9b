"""bloomhip_flush_cuts on the GPU: where the reference's buffer flushes in an
op stream (src/buffer.cpp:37-58, src/lsm_tree.cpp:104-139), against the plain
Python model of tests/tree_model.py.  Edges are placed by the walk's chunk
(bloomhip.TREE_CUT_CHUNK): the last lane of a wave, the first lane of the next,
the last and the first op of a chunk."""
import ctypes

import numpy as np
import pytest

import bloomhip as bh
from tree_model import stream_cuts

pytestmark = pytest.mark.gpu

C = bh.TREE_CUT_CHUNK
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def ops_of(keys):
    keys = np.asarray(keys, dtype=np.int64)
    ops = np.empty((keys.size, 2), dtype=np.int32)
    ops[:, 0] = keys
    ops[:, 1] = np.arange(keys.size) % 1000
    return ops


def check(keys, B, device_ops=False):
    ops = ops_of(keys)
    want = stream_cuts(ops[:, 0].tolist(), B)
    if device_ops:
        import torch
        dev = torch.from_numpy(ops).cuda()
        got = bh.flush_cuts(dev, B)
    else:
        got = bh.flush_cuts(ops, B)
    assert got.dtype == np.uint64
    assert got.tolist() == want, (B, len(keys), got[:8], want[:8])
    return want


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, C - 1, C, C + 1])
def test_distinct_keys(B):
    n = 4 * C + 3
    rng = np.random.default_rng(B)
    keys = rng.permutation(np.arange(n)) - n // 2
    want = check(keys, B)
    assert want == list(range(B, n, B))


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, C - 1, C, C + 1])
@pytest.mark.parametrize("domain", ["B", "B+1", "2B"])
def test_repeated_keys(B, domain):
    """Keys from exactly B, B + 1 and 2B values: segments run many chunks
    long, and the refused op is mostly a key the buffer already holds."""
    d = {"B": B, "B+1": B + 1, "2B": 2 * B}[domain]
    # drawing all of B values takes about B ln B draws: enough for a few cuts
    n = 4 * C + 3 if B <= 65 else 16 * C + 3
    rng = np.random.default_rng(1000 + B)
    keys = rng.integers(0, d, size=n) * 7919 - 3_000_000
    want = check(keys, B)
    if domain == "B" and B > 1:
        # every key is in the full buffer: each refused op is a key it holds
        assert want and all(len(set(keys[a:c].tolist())) == B for a, c in zip([0] + want, want))


def test_stream_edges():
    B = 100
    base = np.arange(B) * 3
    # ends exactly on the B-th distinct key: that cut is not realised
    assert check(base, B) == []
    assert check(np.concatenate([base[:50], base[:50], base]), B) == []
    # one more op, even on a key in the buffer: it is
    assert check(np.concatenate([base, base[:1]]), B) == [B]
    assert check(np.concatenate([base[:50], base[:50], base, [7]]), B) == [200]
    # n <= B, n == 0
    assert check(base[:B - 1], B) == []
    assert check(base[:0], B) == []
    assert check(base[:1], 1) == []
    # the first B ops already distinct (a full buffer carried in), then more
    rng = np.random.default_rng(5)
    assert check(np.concatenate([base, rng.integers(0, 250, size=3000)]), B)[0] == B


def test_extreme_keys_and_all_equal():
    rng = np.random.default_rng(6)
    pool = np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX], dtype=np.int64)
    keys = pool[rng.integers(0, pool.size, size=2 * C + 17)]
    for B in (1, 3, 6, 7):
        check(keys, B)
    for k in (I32_MIN, I32_MAX, 0):
        assert check(np.full(3 * C + 1, k), 2) == []
        assert check(np.full(70, k), 1) == list(range(1, 70))


def test_device_ops():
    pytest.importorskip("torch")
    rng = np.random.default_rng(7)
    for B in (64, C):
        check(rng.integers(-2 * B, 2 * B, size=4 * C + 3), B, device_ops=True)


def test_cuts_cap_too_small():
    keys = np.arange(1000)
    ops = ops_of(keys)
    with pytest.raises(bh.BloomHipError) as ei:
        bh.flush_cuts(ops, 10, cuts_cap=50)
    assert ei.value.status == bh.ERANGE and ei.value.ncuts == 99
    # nothing written, the true count returned
    L = bh.lib()
    cuts = np.full(98, 77, dtype=np.uint64)
    nc = ctypes.c_size_t()
    rc = L.bloomhip_flush_cuts(ops.ctypes.data, 1000, 0, 10, cuts.ctypes.data, 98, ctypes.byref(nc), 0, None)
    assert rc == bh.ERANGE and nc.value == 99 and (cuts == 77).all()
    rc = L.bloomhip_flush_cuts(ops.ctypes.data, 1000, 0, 10, None, 0, ctypes.byref(nc), 0, None)
    assert rc == bh.ERANGE and nc.value == 99
    assert bh.flush_cuts(ops, 10, cuts_cap=99).tolist() == list(range(10, 1000, 10))
    assert L.bloomhip_flush_cuts(ops.ctypes.data, 1000, 0, 10, cuts.ctypes.data, 98, ctypes.byref(nc),
                                 bh.device_count(), None) == bh.EINVAL


def test_tiled_sort_path():
    """More ops than one workgroup sorts: the links come from the tiled radix
    sort, several tiles and all four digit passes."""
    n = 3 * bh.FLUSH_BLOCK_CAP + 5
    rng = np.random.default_rng(8)
    keys = rng.integers(-2**31, 2**31, size=n // 4)[rng.integers(0, n // 4, size=n)]
    want = check(keys, 1000)
    assert len(want) >= 3
