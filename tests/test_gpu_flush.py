"""GPU parity of the batched PUT (bloomhip_flush_batch): a batch of puts and
deletes in arrival order sorted into a run (Buffer::put, src/buffer.cpp:37-58,
walked in key order by a flush, src/lsm_tree.cpp:124-131).

The model is a Python dictionary filled in op order, then sorted by key, with
tombstones removed when drop_tombstones is set.  An op's value is its index
(except tombstones), so a wrong winner among duplicates shows as such.  Every
comparison is exact."""
import ctypes

import numpy as np
import pytest

import bloomhip as bh

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2**31, 2**31 - 1
T, C = bh.FLUSH_TILE, bh.FLUSH_BLOCK_CAP
SCAN_TILES = bh.FLUSH_SCAN_CHUNK // 256  # tiles whose [digit][tile] counts fill one scan chunk
SENTINEL = 0x5A5A5A5A


def make_ops(keys, deletes=None):
    """ops [n, 2]: value = the op's index, INT32_MIN where `deletes` is set."""
    keys = np.asarray(keys, dtype=np.int64)
    ops = np.empty((keys.size, 2), dtype=np.int32)
    ops[:, 0] = keys.astype(np.int32)
    ops[:, 1] = np.arange(keys.size, dtype=np.int32)
    if deletes is not None:
        ops[np.asarray(deletes, dtype=bool), 1] = I32_MIN
    return ops


def model(ops, drop=False):
    d = {}
    for k, v in zip(ops[:, 0].tolist(), ops[:, 1].tolist()):
        d[k] = v  # a second put of a key replaces the first
    run = sorted((k, v) for k, v in d.items() if not (drop and v == I32_MIN))
    return np.array(run, dtype=np.int32).reshape(-1, 2)


def paths_for(n):
    """Both paths where one workgroup could take the batch."""
    return ["auto", "tiled"] if n <= C else ["auto"]


def check(monkeypatch, ops, path, drops=(False, True), **kw):
    monkeypatch.setenv("BLOOMHIP_FLUSH_PATH", path)
    for drop in drops:
        want = model(ops, drop)
        got = bh.flush_batch(ops, drop_tombstones=drop, **kw)
        assert got.shape == want.shape, (path, drop, got.shape, want.shape)
        assert np.array_equal(got, want), (path, drop)


# 512 / 513: the one-workgroup kernel gives every wave one round, then two;
# SCAN_TILES * T (+ 1): the tile counts fill one scan chunk, then need a second
SIZES = sorted({0, 1, 2, 63, 64, 65, 512, 513, T - 1, T, T + 1, 3 * T + 17, C - 1, C, C + 1,
                SCAN_TILES * T, SCAN_TILES * T + 1})


@pytest.mark.parametrize("n", SIZES)
def test_sizes_uniform_keys(monkeypatch, n):
    rng = np.random.default_rng(1000 + n)
    keys = rng.integers(I32_MIN, I32_MAX, size=n, endpoint=True)
    if n > 8:  # some keys written more than once, some deleted
        keys[rng.integers(0, n, size=n // 4)] = keys[rng.integers(0, n, size=n // 4)]
    ops = make_ops(keys, rng.random(n) < 0.1)
    for path in paths_for(n):
        check(monkeypatch, ops, path)


def _patterns(n, rng):
    asc = np.sort(rng.choice(np.arange(-3 * n, 3 * n), size=n, replace=False))
    ext = np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX])
    return {
        "uniform": rng.integers(I32_MIN, I32_MAX, size=n, endpoint=True),
        "extremes": ext[rng.integers(0, ext.size, size=n)],
        "one_key": np.full(n, 123456789),
        "37_keys": rng.integers(I32_MIN, I32_MAX, size=37, endpoint=True)[rng.integers(0, 37, size=n)],
        "low_byte": 0x12345600 + rng.integers(0, 256, size=n),
        "high_byte": (rng.integers(-128, 128, size=n) << 24) + 0x00ABCDEF,
        "sign_only": np.where(rng.random(n) < 0.5, 0x1234567, 0x1234567 - 2**31),
        "ascending": asc,
        "descending": asc[::-1],
        "ascending_twice": np.repeat(asc[: (n + 1) // 2], 2)[:n],
    }


# 3T + 17 ops span more than 3 tiles (the tiled path); 2T - 29 fit one
# workgroup, and go through both paths
@pytest.mark.parametrize("n", [3 * T + 17, 2 * T - 29])
@pytest.mark.parametrize("name", ["uniform", "extremes", "one_key", "37_keys", "low_byte", "high_byte",
                                  "sign_only", "ascending", "descending", "ascending_twice"])
def test_key_patterns(monkeypatch, name, n):
    rng = np.random.default_rng(77)
    keys = _patterns(n, rng)[name]
    assert keys.size == n
    for deletes in (None, rng.random(n) < 0.2):
        ops = make_ops(keys, deletes)
        for path in paths_for(n):
            check(monkeypatch, ops, path, drops=(False,) if deletes is None else (False, True))


@pytest.mark.parametrize("n", [6, 3 * T + 18])
def test_tombstones(monkeypatch, n):
    keys = np.arange(n) * 7 - 3 * n
    third = n // 3
    # put then delete | delete then put | delete only
    k = np.concatenate([keys[:third], keys[third:2 * third], keys[:third], keys[third:2 * third],
                        keys[2 * third:]])
    dels = np.concatenate([np.zeros(third), np.ones(third), np.ones(third), np.zeros(third),
                           np.ones(n - 2 * third)]).astype(bool)
    ops = make_ops(k, dels)
    for path in paths_for(ops.shape[0]):
        check(monkeypatch, ops, path)
        want = model(ops, True)
        assert want.shape[0] == third and set(want[:, 0].tolist()) == set(keys[third:2 * third].tolist())
    # every op a delete
    ops = make_ops(np.random.default_rng(5).integers(-50, 50, size=n), np.ones(n, dtype=bool))
    for path in paths_for(n):
        check(monkeypatch, ops, path)
        monkeypatch.setenv("BLOOMHIP_FLUSH_PATH", path)
        assert bh.flush_batch(ops, drop_tombstones=True).shape == (0, 2)


@pytest.mark.parametrize("n", [1000, C + 1])
def test_buffers(monkeypatch, n):
    import torch
    rng = np.random.default_rng(n)
    ops = make_ops(rng.integers(-n // 3, n // 3, size=n), rng.random(n) < 0.15)
    d_ops = torch.from_numpy(ops).cuda()
    for path in paths_for(n):
        monkeypatch.setenv("BLOOMHIP_FLUSH_PATH", path)
        for drop in (False, True):
            want = model(ops, drop)
            k = want.shape[0]
            # host in / host out, with and without a caller's buffer
            assert np.array_equal(bh.flush_batch(ops, drop_tombstones=drop), want)
            h_out = np.full((n, 2), SENTINEL, dtype=np.int32)
            got = bh.flush_batch(ops, drop_tombstones=drop, out=h_out)
            assert np.array_equal(got, want) and (h_out[k:] == SENTINEL).all()
            # device in / device out: rows at or past n_out untouched, input intact
            d_out = torch.full((n, 2), SENTINEL, dtype=torch.int32, device="cuda")
            got = bh.flush_batch(d_ops, drop_tombstones=drop, out=d_out)
            assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
            assert (d_out[k:] == SENTINEL).all().item()
            assert np.array_equal(d_ops.cpu().numpy(), ops)
            # the same call again: the same answer
            d_out2 = torch.full((n, 2), SENTINEL, dtype=torch.int32, device="cuda")
            bh.flush_batch(d_ops, drop_tombstones=drop, out=d_out2)
            assert torch.equal(d_out, d_out2)
            # mixed
            assert np.array_equal(bh.flush_batch(d_ops, drop_tombstones=drop), want)
            d_out3 = torch.full((n, 2), SENTINEL, dtype=torch.int32, device="cuda")
            got = bh.flush_batch(ops, drop_tombstones=drop, out=d_out3)
            assert np.array_equal(got.cpu().numpy(), want) and (d_out3[k:] == SENTINEL).all().item()


@pytest.mark.parametrize("distinct", [4095, 4096, 4097])
def test_filter_and_metadata(monkeypatch, distinct):
    rng = np.random.default_rng(distinct)
    keys = rng.choice(np.arange(-10**6, 10**6), size=distinct, replace=False)
    k = np.concatenate([keys, keys[rng.integers(0, distinct, size=500)]])
    rng.shuffle(k)
    ops = make_ops(k)
    want = model(ops)
    assert want.shape[0] == distinct
    ref = bh.BloomFilter(bh.m_bits(distinct, 10.0))
    ref.set_batch_run(np.ascontiguousarray(want[:, 0]))
    for path in paths_for(ops.shape[0]):
        monkeypatch.setenv("BLOOMHIP_FLUSH_PATH", path)
        f = bh.BloomFilter(bh.m_bits(distinct, 10.0))
        got = bh.flush_batch(ops, filter=f)
        assert np.array_equal(got, want)
        assert np.array_equal(f.words(), ref.words())
        fences, max_key = f.run_meta()
        rf, rm = ref.run_meta()
        assert np.array_equal(fences, rf) and max_key == rm
        assert fences.size == (distinct + 4095) // 4096


def test_filter_with_tombstones_dropped_and_no_ops(monkeypatch):
    n = 3000
    rng = np.random.default_rng(9)
    ops = make_ops(rng.integers(-2000, 2000, size=n), rng.random(n) < 0.3)
    for path in ("auto", "tiled"):
        monkeypatch.setenv("BLOOMHIP_FLUSH_PATH", path)
        want = model(ops, True)
        f = bh.BloomFilter(bh.m_bits(n, 10.0))
        assert np.array_equal(bh.flush_batch(ops, drop_tombstones=True, filter=f), want)
        ref = bh.BloomFilter(bh.m_bits(n, 10.0))
        ref.set_batch_run(np.ascontiguousarray(want[:, 0]))
        assert np.array_equal(f.words(), ref.words())
        assert np.array_equal(f.run_meta()[0], ref.run_meta()[0]) and f.run_meta()[1] == ref.run_meta()[1]
        # no ops: the filter is cleared and holds the metadata of no keys
        got = bh.flush_batch(np.zeros((0, 2), dtype=np.int32), filter=f)
        assert got.shape == (0, 2)
        empty = bh.BloomFilter(bh.m_bits(n, 10.0))
        empty.set_batch_run(np.zeros(0, dtype=np.int32))
        assert not f.words().any()
        assert np.array_equal(f.run_meta()[0], empty.run_meta()[0]) and f.run_meta()[1] == empty.run_meta()[1]


def test_filter_on_another_device_is_refused():
    f = bh.BloomFilter(1024, device=0)
    ops = make_ops([3, 1, 2])
    out = np.zeros((3, 2), dtype=np.int32)
    n_out = ctypes.c_size_t(77)
    rc = bh.lib().bloomhip_flush_batch(ops.ctypes.data, 3, 0, 0, out.ctypes.data, ctypes.byref(n_out), 0,
                                       f.handle, 1, None)
    assert rc == bh.EINVAL and n_out.value == 77


def test_end_to_end_two_flushed_runs(monkeypatch):
    monkeypatch.setenv("BLOOMHIP_FLUSH_PATH", "auto")
    rng = np.random.default_rng(2024)
    n_old, n_new = 3 * T + 5, 2 * T + 11
    old_ops = make_ops(rng.integers(-20000, 20000, size=n_old))
    new_keys = np.concatenate([old_ops[rng.integers(0, n_old, size=n_new // 2), 0].astype(np.int64),
                               rng.integers(-20000, 20000, size=n_new - n_new // 2)])
    rng.shuffle(new_keys)
    new_ops = make_ops(new_keys, rng.random(n_new) < 0.3)
    new_ops[new_ops[:, 1] != I32_MIN, 1] += 10**6  # newer values differ from older ones
    runs, ents = [], []
    for ops in (new_ops, old_ops):  # newest first
        f = bh.BloomFilter(bh.m_bits(ops.shape[0], 10.0))
        ents.append(bh.flush_batch(ops, filter=f).copy())
        runs.append(f)
    d = {}
    for ops in (old_ops, new_ops):
        for k, v in zip(ops[:, 0].tolist(), ops[:, 1].tolist()):
            d[k] = v
    deleted = [k for k, v in d.items() if v == I32_MIN]
    assert deleted and any(k in set(old_ops[:, 0].tolist()) for k in deleted)
    present = [k for k, v in d.items() if v != I32_MIN][:3000]
    absent = [k for k in range(-21000, 21000, 7) if k not in d]
    q = np.array(present + deleted + absent, dtype=np.int32)
    vals, found, _ = bh.get_batch(runs, ents, q)
    want = np.array([d.get(k, I32_MIN) for k in q.tolist()], dtype=np.int32)
    assert np.array_equal(vals, want)  # a tombstone and a miss both read INT32_MIN
    assert (found[len(present) + len(deleted):] == -1).all()
    assert (found[:len(present) + len(deleted)] >= 0).all()
    # RANGE over both runs
    live = np.array(sorted((k, v) for k, v in d.items() if v != I32_MIN), dtype=np.int32).reshape(-1, 2)
    starts = np.array([I32_MIN, -20000, -5, 0, 100, 19000], dtype=np.int32)
    ends = np.array([I32_MAX, -19000, 5, 0, 5000, I32_MAX], dtype=np.int32)
    off, out = bh.range_batch(runs, ents, starts, ends)
    lo = np.searchsorted(live[:, 0], starts.astype(np.int64))
    hi = np.maximum(np.searchsorted(live[:, 0], ends.astype(np.int64)), lo)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint64))
    assert np.array_equal(out, np.concatenate([live[a:b] for a, b in zip(lo, hi)]))
    # compaction of the two runs == one flush of the older ops then the newer
    both = np.concatenate([old_ops, new_ops])
    for drop in (False, True):
        assert np.array_equal(bh.compact(ents, drop_tombstones=drop),
                              bh.flush_batch(both, drop_tombstones=drop))
        assert np.array_equal(bh.flush_batch(both, drop_tombstones=drop), model(both, drop))
