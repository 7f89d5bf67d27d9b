"""Compaction at the edges of both of its device paths (csrc/bloom_merge.hip),
bit-exact against the C oracle and the numpy model of tests/merge_model.py,
whose inputs tests/test_merge_model_host.py proves to sit on their edges.

* The one-pass k-way kernels (up to 8 runs), forced through
  ubench_kway_compact, which also returns the partition bounds: run lengths
  around the 256-entry sample stride, total sample counts around the
  partition's q = 32 - k samples, the fullest partition there can be
  (q * 256 + (k - 1) * 255 entries, for every k), a partition boundary inside
  one key's entries (INT32_MIN among them: the predecessor's key equals the
  "no predecessor" default), partitions that keep nothing inside the
  look-back, disjoint key ranges (empty shares), runs at odd address parity.
* A merge round (ubench_merge_round) against the model's stable merge: one
  pair at the 2,048-output tile's edges, every key pattern, both address
  parities of either input; rounds of 2, 7 and 8 pairs, one with a pair of no
  entries; 9 pairs refused.
* The dedup (ubench_dedup) against numpy: sizes around its 16-byte vector,
  512-entry round and 4,096-entry tile, equal keys across each of them, and
  1,025 and 1,026 tiles, where k_scan_counts takes its second chunk and
  carries the first chunk's total into it.
* bloomhip_compact with 9 to 64 runs (the pairwise rounds: odd runs copied
  at several depths, 8 pairs, 9 pairs in two launches, 32 pairs), device
  runs at odd parity (stage_share's unaligned vectors), 64 runs of one key,
  and 4.2 million entries through the scan's second chunk.

Values encode run << 24 | index, so a wrong winner among equal keys shows.
"""
import ctypes
import os

import numpy as np
import pytest

import bloomhip as bh
import merge_model as mm

pytestmark = pytest.mark.gpu
SENT = -0x5A5A5A5B  # fills the outputs: what a kernel must not touch stays this
HIP_INVALID_VALUE = 1


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ub():
    bh.lib()  # torch's HIP runtime first (bloomhip._lib): one runtime per process
    L = ctypes.CDLL(os.path.join(os.path.dirname(bh.LIB_PATH), "libbloomhip_ubench.so"))
    P = ctypes.c_void_p
    L.ubench_kway_compact.argtypes = [P, P, ctypes.c_int, ctypes.c_int, P, P, P, P, P]
    L.ubench_merge_round.argtypes = [P] * 5 + [ctypes.c_int]
    L.ubench_dedup.argtypes = [P, ctypes.c_uint64, ctypes.c_int, P, P, P]
    return L


def _dev(torch, e, odd=False):
    """The entries on the device, starting at a 16-byte boundary or 8 bytes past one."""
    n = e.shape[0]
    buf = torch.zeros((n + 2, 2), dtype=torch.int32, device="cuda")
    view = buf[1:1 + n] if odd else buf[:n]
    view.copy_(torch.from_numpy(e))
    if n:
        assert view.data_ptr() % 16 == (8 if odd else 0)
    return view


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# --------------------------------------------------------------------------
# the one-pass k-way kernels
# --------------------------------------------------------------------------
def _kway(torch, ub, runs, drop, odd):
    d = [_dev(torch, r, odd) for r in runs]
    k, total = len(runs), sum(r.shape[0] for r in runs)
    ns = np.array([r.shape[0] for r in runs], dtype=np.uint64)
    out = torch.full((total + 2, 2), SENT, dtype=torch.int32, device="cuda")
    keys = torch.full((total + 2,), SENT, dtype=torch.int32, device="cuda")
    bounds = np.full((sum(mm.nsamples(int(n)) for n in ns) + 1, mm.MAX_RUNS), 0xFFFFFFFF, dtype=np.uint32)
    nparts, count = ctypes.c_uint64(), ctypes.c_uint32()
    torch.cuda.synchronize()
    rc = ub.ubench_kway_compact(_ptrs(d), ns.ctypes.data, k, int(drop), out.data_ptr(), keys.data_ptr(),
                                bounds.ctypes.data, ctypes.byref(nparts), ctypes.byref(count))
    assert rc == 0, rc
    return (bounds[:nparts.value + 1, :k].astype(np.int64), out.cpu().numpy(), keys.cpu().numpy(),
            count.value)


def _check_kway(torch, ub, coracle, runs, odd=False):
    for drop in (False, True):
        st = mm.kway_stats(runs, drop)
        assert st["sizes"].max() <= mm.CAP  # the model's partitions fit the kernel's buffer
        bounds, out, keys, count = _kway(torch, ub, runs, drop, odd)
        want = coracle.compact(runs, drop)
        assert np.array_equal(bounds, st["bounds"])
        assert count == want.shape[0] == st["kept"].sum()
        assert np.array_equal(out[:count], want)
        assert np.array_equal(keys[:count], want[:, 0])
        assert (out[count:] == SENT).all() and (keys[count:] == SENT).all()


def _check_meta(coracle, f, want):
    fences, mk = f.run_meta()
    if want.shape[0]:
        assert (f.words() == coracle.build(f.m, want[:, 0].copy())).all()
        wf, wmk = coracle.run_meta(want[:, 0].copy())
        assert np.array_equal(fences, wf) and mk == wmk
    else:  # an empty run: no bits, no fences, the metadata of no keys
        assert not f.words().any()
        assert fences.size == 0 and mk == mm.I32_MIN


def _check_api(coracle, runs, given=None, out=None):
    """bloomhip_compact with a fused filter, both tombstone modes; `given`:
    the runs as the call gets them (device views), `out` a device buffer."""
    total = sum(r.shape[0] for r in runs)
    for drop in (False, True):
        f = bh.BloomFilter(bh.m_bits(max(total, 1), 10.0))
        got = bh.compact(given if given is not None else runs, drop_tombstones=drop, filter=f, out=out)
        got = got.cpu().numpy() if out is not None else np.asarray(got)
        want = coracle.compact(runs, drop)
        assert np.array_equal(got.reshape(-1, 2), want)
        _check_meta(coracle, f, want)


@pytest.mark.parametrize("sizes", mm.RUN_LENGTHS, ids=lambda s: "-".join(map(str, s)))
def test_kway_run_lengths_around_the_sample_stride(torch, ub, coracle, sizes):
    runs = mm.run_length_case(sizes)
    _check_kway(torch, ub, coracle, runs)
    _check_api(coracle, runs)


@pytest.mark.parametrize("which", mm.SAMPLE_COUNTS)
@pytest.mark.parametrize("k", mm.SAMPLE_KS)
def test_kway_sample_counts_around_a_partition(torch, ub, coracle, k, which):
    runs = mm.sample_count_case(k, which)
    assert mm.kway_stats(runs, False)["nparts"] == {"q-1": 1, "q": 1, "q+1": 2, "2q": 2, "2q+1": 3}[which]
    _check_kway(torch, ub, coracle, runs)


@pytest.mark.parametrize("a_newest", [True, False], ids=["a_newest", "a_oldest"])
@pytest.mark.parametrize("k", range(1, mm.MAX_RUNS + 1))
def test_kway_fullest_partition(torch, ub, coracle, k, a_newest):
    runs = mm.fullest_partition_case(k, a_newest)
    assert mm.kway_stats(runs, False)["sizes"][1] == mm.max_partition(k)
    _check_kway(torch, ub, coracle, runs)
    _check_api(coracle, runs)


@pytest.mark.parametrize("tomb", [False, True], ids=["live", "tombstone"])
@pytest.mark.parametrize("key", mm.EQUAL_KEYS)
def test_kway_boundary_inside_equal_keys(torch, ub, coracle, key, tomb):
    runs = mm.equal_keys_case(key, tomb)
    _check_kway(torch, ub, coracle, runs)
    want = coracle.compact(runs, True)
    assert want.shape[0] == (0 if tomb else 1)  # with tombstones dropped: one entry, or none


def test_kway_partitions_that_keep_nothing(torch, ub, coracle):
    runs = mm.tombstone_stretch_case()
    kept = mm.kway_stats(runs, True)["kept"]
    assert ((kept[1:] == 0) & (kept[:-1] == 0)).any() and kept[0] > 0 and kept[-1] > 0
    _check_kway(torch, ub, coracle, runs)


@pytest.mark.parametrize("descending", [True, False], ids=["descending", "ascending"])
@pytest.mark.parametrize("n", [5000, 8000])
def test_kway_disjoint_key_ranges(torch, ub, coracle, n, descending):
    # a partition is q = 28 samples, 7,168 entries: at 5,000 entries a run every
    # partition spans two runs (two of its four shares empty); at 8,000 some
    # lie inside one run (three empty), test_merge_model_host.py::test_disjoint_cases
    _check_kway(torch, ub, coracle, mm.disjoint_case(n, descending))


@pytest.mark.parametrize("case", ["run_lengths", "fullest"])
def test_kway_runs_at_odd_address_parity(torch, ub, coracle, case):
    runs = (mm.run_length_case(mm.RUN_LENGTHS[-1]) if case == "run_lengths"
            else mm.fullest_partition_case(8, False))
    _check_kway(torch, ub, coracle, runs, odd=True)


# --------------------------------------------------------------------------
# a merge round
# --------------------------------------------------------------------------
def _merge_round(torch, ub, pairs, par_a=0, par_b=0, want_rc=0):
    """The pairs' outputs share one buffer, each at an even entry (as
    compact_device lays them out), two untouched entries after the last."""
    offs, o = [], 0
    for a, b in pairs:
        offs.append(o)
        o += (a.shape[0] + b.shape[0] + 1) & ~1
    out = torch.full((o + 2, 2), SENT, dtype=torch.int32, device="cuda")
    da = [_dev(torch, a, par_a) for a, _ in pairs]
    db = [_dev(torch, b, par_b) for _, b in pairs]
    na = np.array([a.shape[0] for a, _ in pairs], dtype=np.uint64)
    nb = np.array([b.shape[0] for _, b in pairs], dtype=np.uint64)
    po = (ctypes.c_void_p * len(pairs))(*[out.data_ptr() + 8 * x for x in offs])
    torch.cuda.synchronize()
    rc = ub.ubench_merge_round(_ptrs(da), na.ctypes.data, _ptrs(db), nb.ctypes.data, po, len(pairs))
    assert rc == want_rc, rc
    got = out.cpu().numpy()
    if want_rc:
        assert (got == SENT).all()
        return
    ends = offs[1:] + [o + 2]
    for (a, b), off, end in zip(pairs, offs, ends):
        t = a.shape[0] + b.shape[0]
        assert np.array_equal(got[off:off + t], mm.merge2(a, b))
        assert (got[off + t:end] == SENT).all()  # the padding of an odd total, the sentinels


@pytest.mark.parametrize("pattern", mm.PAIR_PATTERNS)
@pytest.mark.parametrize("na,nb", mm.PAIR_SIZES)
def test_merge_round_one_pair(torch, ub, na, nb, pattern):
    pair = mm.pair_case(na, nb, pattern)
    for par_a in (0, 1):
        for par_b in (0, 1):
            _merge_round(torch, ub, [pair], par_a, par_b)


@pytest.mark.parametrize("npairs,empty_at", [(2, None), (7, None), (8, None), (7, 3), (8, 7)])
def test_merge_round_of_several_pairs(torch, ub, npairs, empty_at):
    pairs = mm.round_case(npairs, empty_at)
    _merge_round(torch, ub, pairs)
    _merge_round(torch, ub, pairs, 1, 1)


def test_merge_round_of_nothing_and_of_too_many(torch, ub):
    empty = np.empty((0, 2), dtype=np.int32)
    _merge_round(torch, ub, [(empty, empty)])  # success, nothing launched
    _merge_round(torch, ub, [mm.pair_case(1, 1, "equal")] * (mm.MAX_PAIRS + 1), want_rc=HIP_INVALID_VALUE)


# --------------------------------------------------------------------------
# the dedup
# --------------------------------------------------------------------------
def _dedup(torch, ub, d_in, n, drop):
    """(out, keys_out, count) of ubench_dedup on n entries at d_in (a device tensor)."""
    out = torch.full((n + 2, 2), SENT, dtype=torch.int32, device="cuda")
    keys = torch.full((n + 2,), SENT, dtype=torch.int32, device="cuda")
    count = ctypes.c_uint32()
    torch.cuda.synchronize()
    rc = ub.ubench_dedup(d_in.data_ptr(), n, int(drop), out.data_ptr(), keys.data_ptr(), ctypes.byref(count))
    assert rc == 0, rc
    return out, keys, count.value


def _check_dedup(torch, ub, e):
    d_in = _dev(torch, e)
    for drop in (False, True):
        out, keys, count = _dedup(torch, ub, d_in, e.shape[0], drop)
        out, keys = out.cpu().numpy(), keys.cpu().numpy()
        want = mm.dedup(e, drop)
        assert count == want.shape[0]
        assert np.array_equal(out[:count], want) and np.array_equal(keys[:count], want[:, 0])
        assert (out[count:] == SENT).all() and (keys[count:] == SENT).all()


@pytest.mark.parametrize("pattern", mm.DEDUP_PATTERNS)
@pytest.mark.parametrize("n", mm.DEDUP_SIZES)
def test_dedup_at_vector_round_and_tile_edges(torch, ub, n, pattern):
    _check_dedup(torch, ub, mm.dedup_case(n, pattern))


def test_dedup_dropped_tombstone_takes_its_older_copies_along(torch, ub):
    # a tombstone that is the first of its key, live older copies behind it:
    # with tombstones dropped both go, at every position of a vector and
    # across a round and a tile
    keys = np.repeat(np.arange(3000), 2)
    e = mm.entries(keys, 0, np.arange(keys.size) % 6 == 0)
    e2 = mm.entries(np.concatenate([[-1], keys]), 0, np.arange(keys.size + 1) % 6 == 1)
    for arr in (e, e2):
        want = mm.dedup(arr, True)
        assert want.shape[0] < np.unique(arr[:, 0]).size and (want[:, 1] != mm.TOMB).all()
        _check_dedup(torch, ub, arr)


@pytest.mark.parametrize("tiles", [mm.SCAN_CHUNK, mm.SCAN_CHUNK + 1])
def test_dedup_scan_takes_a_second_chunk(torch, ub, tiles):
    # tiles * 4096 + 1 entries are tiles + 1 dedup tiles: 1,025 is the fewest
    # at which k_scan_counts runs a second chunk and adds the first's total
    n = tiles * mm.DEDUP_TILE + 1
    assert -(-n // mm.DEDUP_TILE) > mm.SCAN_CHUNK
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    vals = (i & 0xFFFFFF).to(torch.int32)
    vals[i % 5 == 0] = mm.TOMB
    e = torch.stack([(i // 3).to(torch.int32), vals], dim=1).contiguous()
    first = torch.ones(n, dtype=torch.bool, device="cuda")
    first[1:] = e[1:, 0] != e[:-1, 0]
    for drop in (False, True):
        keep = first & (e[:, 1] != mm.TOMB) if drop else first
        want = e[keep]
        out, keys, count = _dedup(torch, ub, e, n, drop)
        assert count == want.shape[0]
        assert torch.equal(out[:count], want) and torch.equal(keys[:count], want[:, 0])
        assert bool((out[count:] == SENT).all()) and bool((keys[count:] == SENT).all())


# --------------------------------------------------------------------------
# bloomhip_compact with more than 8 runs: the pairwise rounds, then the dedup
# --------------------------------------------------------------------------
@pytest.mark.parametrize("nruns", mm.MANY_RUNS)
def test_compact_many_runs(coracle, nruns):
    _check_api(coracle, mm.many_runs_case(nruns))


@pytest.mark.parametrize("nruns", [9, 17])
def test_compact_many_device_runs_at_odd_address_parity(torch, coracle, nruns):
    # every run 8 bytes past a 16-byte boundary: the merge tile stages the
    # first round's shares from unaligned vectors (stage_share at parity 1)
    runs = mm.many_runs_case(nruns)
    views = [_dev(torch, r, odd=True) for r in runs]
    out = torch.empty((sum(r.shape[0] for r in runs), 2), dtype=torch.int32, device="cuda")
    _check_api(coracle, runs, given=views, out=out)


@pytest.mark.parametrize("newest_is_tombstone", [False, True], ids=["live", "tombstone"])
def test_compact_64_runs_of_one_key(coracle, newest_is_tombstone):
    runs = [mm.entries([42], j) for j in range(64)]
    if newest_is_tombstone:
        runs[0][0, 1] = mm.TOMB
    assert np.array_equal(coracle.compact(runs, False), runs[0])  # the newest wins
    assert coracle.compact(runs, True).shape[0] == (0 if newest_is_tombstone else 1)
    _check_api(coracle, runs)


def test_compact_many_runs_through_the_scans_second_chunk(coracle):
    runs = mm.second_chunk_runs()
    total = sum(r.shape[0] for r in runs)
    assert len(runs) == 9 and -(-total // mm.DEDUP_TILE) > mm.SCAN_CHUNK + 1
    got = bh.compact(runs, drop_tombstones=True)
    assert np.array_equal(got, coracle.compact(runs, True))
