"""GPU parity of the batched RANGE (bloomhip_range_batch): newest-wins range
scans over the runs (LSMTree::range, src/lsm_tree.cpp:218-290).

Expected answers come from a numpy/dictionary model: the runs are applied
oldest first to a dictionary (the newest run's entry of a key wins),
tombstones are dropped, the keys sorted; query [start, end) answers the
model's entries with start <= key < end.  Everything is compared exactly."""
import ctypes
import json
import os

import numpy as np
import pytest

import bloomhip as bh
from test_gpu_get import entries_of
from test_gpu_route import sorted_run

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2**31, 2**31 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def merged_view(ents):
    """The dictionary model over whole runs (newest first): [n, 2] int32,
    keys ascending, tombstones dropped."""
    d = {}
    for e in ents[::-1]:
        d.update(zip(e[:, 0].tolist(), e[:, 1].tolist()))
    live = sorted((k, v) for k, v in d.items() if v != I32_MIN)
    return np.array(live, dtype=np.int32).reshape(-1, 2)


def model(ents, starts, ends, view=None):
    """(offsets, out_entries) the call must return."""
    view = merged_view(ents) if view is None else view
    s = np.asarray(starts, dtype=np.int64)
    e = np.asarray(ends, dtype=np.int64)
    lo = np.searchsorted(view[:, 0], s, side="left")
    hi = np.maximum(np.searchsorted(view[:, 0], e, side="left"), lo)
    hi = np.where(e <= s, lo, hi)
    offsets = np.zeros(s.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(hi - lo)
    parts = [view[a:b] for a, b in zip(lo, hi) if b > a]
    out = np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.int32)
    return offsets, out


def candidates(ents, starts, ends):
    """Per query, the entries of every run inside its bounds."""
    s = np.asarray(starts, dtype=np.int64)
    e = np.asarray(ends, dtype=np.int64)
    ub = np.zeros(s.size, dtype=np.int64)
    for x in ents:
        k = x[:, 0].astype(np.int64)
        ub += np.maximum(np.searchsorted(k, e) - np.searchsorted(k, s), 0) * (e > s)
    return ub


def handle_for(e, meta=True):
    f = bh.BloomFilter(bh.m_bits(max(e.shape[0], 1), 10.0))
    keys = np.ascontiguousarray(e[:, 0])
    if meta:
        f.set_batch_run(keys)
    else:
        f.set_batch(keys)
    return f


def check(runs, ents, starts, ends, view=None, **kw):
    starts = np.asarray(starts, dtype=np.int32)
    ends = np.asarray(ends, dtype=np.int32)
    want_off, want_out = model(ents, starts, ends, view)
    off, out = bh.range_batch(runs, ents, starts, ends, **kw)
    assert np.array_equal(off, want_off)
    assert out.shape == want_out.shape and np.array_equal(out, want_out)
    return want_off, want_out


def edge_bounds(ents):
    """Queries around every run's first and last key and the first and last
    key of every fence interval (and their +-1 neighbours): one-key ranges,
    empty and reversed ones, neighbour to neighbour, the int32 extremes, the
    full domain, and duplicated queries."""
    pts = [np.array([I32_MIN, I32_MIN + 1, I32_MAX - 1, I32_MAX], dtype=np.int64)]
    for e in ents:
        k = e[:, 0].astype(np.int64)
        if k.size == 0:
            continue
        b = np.concatenate([k[:1], k[-1:], k[::4096], k[4095::4096]])
        pts.append(np.concatenate([b - 1, b, b + 1]))
    p = np.unique(np.clip(np.concatenate(pts), I32_MIN, I32_MAX))
    nxt = np.minimum(p + 1, I32_MAX)
    s = [p, p, p[:-1], nxt, p[:-2]]
    e = [nxt, p, p[1:], p, p[2:]]          # one key; start == end; neighbours; end < start; wider
    s.append(np.array([I32_MIN, I32_MIN, I32_MAX, I32_MAX, I32_MAX - 1, 0, I32_MIN], dtype=np.int64))
    e.append(np.array([I32_MAX, I32_MIN, I32_MAX, I32_MIN, I32_MAX, 0, 0], dtype=np.int64))
    s, e = np.concatenate(s), np.concatenate(e)
    s, e = np.concatenate([s, s[:70]]), np.concatenate([e, e[:70]])  # duplicated queries
    return s.astype(np.int32), e.astype(np.int32)


RUN_SIZES = [0, 1, 511, 512, 513, 4095, 4096, 4097, 12_289]
NO_HANDLE = 4  # the run passed with a None handle


@pytest.fixture(scope="module")
def sized():
    """One run of every size of RUN_SIZES, built once and left unchanged: the
    empty one without metadata, one with a None handle, a tombstone in every
    tenth entry of the larger ones."""
    ents, runs = [], []
    for j, n in enumerate(RUN_SIZES):
        e = entries_of(sorted_run(n, 300 + j), 400 + j)
        if n > 100:
            e[::10, 1] = I32_MIN
        ents.append(e)
        runs.append(None if j == NO_HANDLE else handle_for(e, meta=n > 0))
    return runs, ents, merged_view(ents)


def test_run_sizes_and_interval_edges(sized):
    runs, ents, view = sized
    s, e = edge_bounds(ents)
    off, out = check(runs, ents, s, e, view)
    assert candidates(ents, s, e).max() > bh.RANGE_BLOCK_CAP and out.shape[0] > 30_000
    for j in range(len(ents)):  # each size alone, with its own edges
        sj, ej = edge_bounds(ents[j:j + 1])
        check(runs[j:j + 1], ents[j:j + 1], sj, ej)


def mixed_queries(view, nq, seed, long_every=97):
    """nq queries with 0 to a few thousand results over the merged view."""
    rng = np.random.default_rng(seed)
    n = view.shape[0]
    i = rng.integers(0, n - 1, size=nq)
    span = rng.integers(0, 12, size=nq)
    span[::7] = rng.integers(0, 700, size=span[::7].size)
    span[::long_every] = rng.integers(700, 4000, size=span[::long_every].size)
    j = np.minimum(i + span, n - 1)
    return view[i, 0], view[j, 0]


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 5000])
def test_query_counts(sized, nq):
    runs, ents, view = sized
    s, e = mixed_queries(view, nq, nq + 1)
    off, out = check(runs, ents, s, e, view)
    assert off.size == nq + 1 and off[0] == 0
    if nq == 5000:
        ub = candidates(ents, s, e)
        assert (ub == 0).any() and (ub > bh.RANGE_BLOCK_CAP).any()
        assert ((ub > bh.RANGE_WAVE_CAP) & (ub <= bh.RANGE_BLOCK_CAP)).any()


@pytest.mark.parametrize("path", ["auto", "compact"])
@pytest.mark.parametrize("nruns", [1, 2, 5, 8, 9, 16, 17, 64])
def test_run_counts(nruns, path, monkeypatch):
    """A narrow key domain, so that the runs overlap heavily; 8 and 9 runs
    straddle the k-way limit of the large path."""
    monkeypatch.setenv("BLOOMHIP_RANGE_PATH", path)
    ents, runs = [], []
    for j in range(nruns):
        n = 300 + 7 * j if nruns > 16 else [4097, 600, 9000, 513, 5000][j % 5]
        rng = np.random.default_rng(50 + j)
        keys = np.unique(rng.integers(-20_000, 20_000, size=n, dtype=np.int64).astype(np.int32))
        e = entries_of(keys, 60 + j)
        e[rng.integers(0, keys.size, size=keys.size // 8), 1] = I32_MIN
        ents.append(e)
        runs.append(None if j % 4 == 3 else handle_for(e))
    rng = np.random.default_rng(nruns)
    width = np.array([0, 1, 2, 5, 20, 60, 200, 700, 3000, 15_000, 40_100] * 3)
    s = rng.integers(-20_050, 20_050, size=width.size)
    s[-1] = -20_050
    e = np.minimum(s + width, 20_060)
    off, out = check(runs, ents, s, e)
    ub = candidates(ents, s, e)
    assert ub.max() > bh.RANGE_BLOCK_CAP and out.shape[0] > 0
    if nruns >= 8:
        # the large path meets at least nruns non-empty sub-ranges
        assert max(sum(1 for x in ents if np.searchsorted(x[:, 0], b) > np.searchsorted(x[:, 0], a))
                   for a, b in zip(s, e)) == nruns


def test_class_edges():
    """Candidate counts of exactly cap - 1, cap and cap + 1 for both caps, over
    consecutive-integer keys: run 0 holds 0 .. 3999, run 1 holds 1000 .. 3999,
    so [1000 - j, 1000 + k) has j + 2k candidates."""
    e0 = entries_of(np.arange(0, 4000, dtype=np.int32), 1)
    e1 = entries_of(np.arange(1000, 4000, dtype=np.int32), 2)
    e0[::3, 1] = I32_MIN
    e1[::5, 1] = I32_MIN
    ents = [e0, e1]
    runs = [handle_for(e0), handle_for(e1)]
    targets = [c + d for c in (bh.RANGE_WAVE_CAP, bh.RANGE_BLOCK_CAP) for d in (-1, 0, 1)]
    s, e = [], []
    for t in targets:
        k = (t - 101) // 2
        s.append(1000 - (t - 2 * k))
        e.append(1000 + k)
    s += [0, 0, 0]                      # one run only: 511, 512, 513 candidates
    e += [511, 512, 513]
    assert candidates(ents, s, e).tolist() == targets + [511, 512, 513]
    check(runs, ents, s, e)
    check(runs, ents, s[::-1], e[::-1])
    check(runs[::-1], ents[::-1], s, e)  # the other run the newer one


def test_newest_wins_and_tombstones():
    keys = np.arange(0, 6000, 3, dtype=np.int32)
    ents = []
    for j in range(3):  # one key set in three runs with distinct values
        e = entries_of(keys, 70 + j)
        e[:, 1] = 1000 * (j + 1) + (np.arange(keys.size) % 1000)
        ents.append(e)
    ents[0][5, 1] = I32_MIN      # a tombstone in the newest run over live older values
    ents[1][9, 1] = I32_MIN      # a tombstone under a newer live value
    only_old = np.arange(1, 6000, 3, dtype=np.int32)[:500]
    e3 = entries_of(only_old, 75)
    e3[7, 1] = I32_MIN           # a tombstone in the oldest run alone
    ents.append(e3)
    # keys 3000 .. 3029: tombstones in the newest run, live in the older ones
    hid = (keys >= 3000) & (keys < 3030)
    ents[0][hid, 1] = I32_MIN
    runs = [handle_for(e) for e in ents]
    s = [0, 15, 27, 22, 0, 3000, 3000, 2997, I32_MIN]
    e = [6000, 16, 28, 23, 40, 3030, 3001, 3031, I32_MAX]
    off, out = check(runs, ents, s, e)
    n = np.diff(off.astype(np.int64))
    first = out[off[0]:off[1]]
    own = first[first[:, 0] % 3 == 0]
    assert (own[:, 1] < 2000).all()                       # the newest run's values
    assert n[1] == 0                                      # key 15: hidden by the newest tombstone
    assert n[2] == 1 and out[off[2], 1] == ents[0][9, 1]  # key 27: the newer live value
    assert n[3] == 0                                      # key 22: a tombstone in the oldest run alone
    assert n[5] == 0 and n[6] == 0                        # every candidate hidden or a tombstone
    assert candidates(ents, s[5:6], e[5:6])[0] == 30 and n[7] == 2


def test_heavy_duplicates():
    """The same 300 keys in all 64 runs: the answer is the newest run's."""
    keys = np.arange(-450, 450, 3, dtype=np.int32)
    assert keys.size == 300
    ents = [entries_of(keys, 800 + j) for j in range(64)]
    runs = [handle_for(e) if j % 2 else None for j, e in enumerate(ents)]
    s = [-450, -450, 0, 0, 447, -10_000]
    e = [450, -435, 60, 6, 448, 10_000]
    ub = candidates(ents, s, e)
    assert ub.tolist() == [19_200, 320, 1280, 128, 64, 19_200]
    off, out = check(runs, ents, s, e)
    assert np.array_equal(out[:300], ents[0])


def raw_call(handles, eptrs, sizes, nruns, starts, ends, nq, offsets, out, cap, total, device=0,
             ent_dev=0):
    n = max(len(handles), 1) + 70
    H = (ctypes.c_void_p * n)(*handles)
    E = (ctypes.c_void_p * n)(*eptrs)
    N = (ctypes.c_size_t * n)(*sizes)
    return bh.lib().bloomhip_range_batch(
        H, E, N, nruns, ent_dev, starts, ends, nq, 0, offsets, out, cap,
        ctypes.byref(total) if total is not None else None, 0, device, None)


def test_capacity(sized):
    runs, ents, view = sized
    s, e = mixed_queries(view, 300, 5)
    want_off, want_out = model(ents, s, e, view)
    total_want = want_out.shape[0]
    assert total_want > 100
    hs = [r.handle.value if r is not None else None for r in runs]
    ps = [x.ctypes.data if x.shape[0] else None for x in ents]
    ns = [x.shape[0] for x in ents]
    s, e = np.ascontiguousarray(s), np.ascontiguousarray(e)
    off = np.full(s.size + 1, 7, dtype=np.uint64)
    total = ctypes.c_size_t(99)
    sp, ep = s.ctypes.data, e.ctypes.data
    # count only
    assert raw_call(hs, ps, ns, len(hs), sp, ep, s.size, off.ctypes.data, None, 0, total) == bh.OK
    assert total.value == total_want and np.array_equal(off, want_off)
    # exact capacity
    out = np.full((total_want, 2), 77, dtype=np.int32)
    off[:] = 7
    assert raw_call(hs, ps, ns, len(hs), sp, ep, s.size, off.ctypes.data, out.ctypes.data, total_want,
                    total) == bh.OK
    assert np.array_equal(off, want_off) and np.array_equal(out, want_out)
    # one entry short
    out[:] = 77
    off[:] = 7
    total.value = 99
    assert raw_call(hs, ps, ns, len(hs), sp, ep, s.size, off.ctypes.data, out.ctypes.data, total_want - 1,
                    total) == bh.ERANGE
    assert total.value == total_want and np.array_equal(off, want_off) and (out == 77).all()
    # the binding raises
    with pytest.raises(bh.BloomHipError) as ei:
        bh.range_batch(runs, ents, s, e, out=np.empty((total_want - 1, 2), dtype=np.int32))
    assert ei.value.status == bh.ERANGE
    off2, out2 = bh.range_batch(runs, ents, s, e, out=np.empty((total_want + 5, 2), dtype=np.int32))
    assert np.array_equal(out2, want_out)


@pytest.mark.parametrize("bounds_dev", [False, True], ids=["hostbounds", "devbounds"])
@pytest.mark.parametrize("ent_dev", [False, True], ids=["hostent", "devent"])
@pytest.mark.parametrize("out_dev", [False, True], ids=["hostout", "devout"])
def test_residency(sized, bounds_dev, ent_dev, out_dev):
    torch = pytest.importorskip("torch")
    runs, ents, view = sized
    s, e = edge_bounds(ents)
    want_off, want_out = model(ents, s, e, view)
    sb = torch.from_numpy(s).cuda() if bounds_dev else s
    eb = torch.from_numpy(e).cuda() if bounds_dev else e
    if ent_dev:
        # views at an odd row of a larger tensor: 8-byte aligned, row stride 8
        devs = []
        for x in ents:
            big = torch.zeros((x.shape[0] + 3, 2), dtype=torch.int32, device="cuda")
            big[3:] = torch.from_numpy(x)
            v = big[3:]
            assert v.stride(0) * v.element_size() == 8
            assert x.shape[0] == 0 or v.data_ptr() % 16 == 8
            devs.append(v)
    else:
        devs = ents
    torch.cuda.synchronize()
    if out_dev:
        offs = torch.empty(s.size + 1, dtype=torch.int64, device="cuda")
        off, out = bh.range_batch(runs, devs, sb, eb, offsets=offs)
        assert out.is_cuda and off.is_cuda
        off, out = off.cpu().numpy().view(np.uint64), out.cpu().numpy()
        # and into a caller's buffer
        buf = torch.full((want_out.shape[0] + 1, 2), 9, dtype=torch.int32, device="cuda")
        off2, out2 = bh.range_batch(runs, devs, sb, eb, out=buf)
        assert np.array_equal(out2.cpu().numpy(), want_out) and (buf[-1] == 9).all()
        assert np.array_equal(off2.cpu().numpy().view(np.uint64), want_off)
    else:
        off, out = bh.range_batch(runs, devs, sb, eb)
    assert np.array_equal(off, want_off) and np.array_equal(out, want_out)


def test_argument_errors():
    e = entries_of(np.arange(5000, dtype=np.int32), 1)
    f = bh.BloomFilter(1000)
    f.set_batch_run(np.ascontiguousarray(e[:, 0]))  # 2 fences
    f.profile(True)
    f.profile_reset()
    s = np.array([0, 10], dtype=np.int32)
    en = np.array([5, 5000], dtype=np.int32)
    off = np.full(3, 7, dtype=np.uint64)
    out = np.full((6000, 2), 77, dtype=np.int32)
    total = ctypes.c_size_t(99)
    h, p = f.handle.value, e.ctypes.data
    sp, ep, op, bp = s.ctypes.data, en.ctypes.data, off.ctypes.data, out.ctypes.data

    def call(handles=(h,), eptrs=(p,), sizes=(5000,), nruns=1, starts=sp, ends=ep, offsets=op, buf=bp,
             cap=6000, tot=total, device=0, ent_dev=0):
        return raw_call(list(handles), list(eptrs), list(sizes), nruns, starts, ends, 2, offsets, buf, cap,
                        tot, device, ent_dev)

    assert call() == bh.OK
    assert total.value == 4995 and off.tolist() == [0, 5, 4995]
    off[:] = 7
    out[:] = 77
    total.value = 99
    f.profile_reset()
    assert call(starts=None) == bh.EINVAL
    assert call(ends=None) == bh.EINVAL
    assert call(offsets=None) == bh.EINVAL
    assert call(tot=None) == bh.EINVAL
    assert call(buf=None) == bh.EINVAL                    # no buffer for a capacity
    assert call(eptrs=(None,)) == bh.EINVAL               # NULL entries, nentries > 0
    assert call(eptrs=(p + 2,)) == bh.EINVAL              # misaligned host entries
    assert call(eptrs=(p + 4,), ent_dev=1) == bh.EINVAL   # device entries are read as 8-byte words
    assert call(sizes=(4096,)) == bh.EINVAL               # 2 fences, entries for 1
    assert call(sizes=(8193,)) == bh.EINVAL               # entries for 3
    assert call(nruns=0) == bh.EINVAL
    assert call(handles=[h] * 65, eptrs=[p] * 65, sizes=[5000] * 65, nruns=65) == bh.EINVAL
    assert call(device=-1) == bh.EINVAL
    assert call(device=bh.device_count()) == bh.EINVAL
    if bh.device_count() > 1:
        g = bh.BloomFilter(1000, device=1)
        assert call(handles=(h, g.handle.value), eptrs=(p, None), sizes=(5000, 0), nruns=2) == bh.EINVAL
    assert (off == 7).all() and (out == 77).all() and total.value == 99
    assert f.profile_read() == {}
    f.profile(False)
    # a handle without metadata and a NULL handle take any entries
    assert call(handles=(None,), sizes=(4096,)) == bh.OK
    assert total.value == 4091 and off.tolist() == [0, 5, 4091]


def test_runs_on_two_devices_refused():
    if bh.device_count() < 2:
        pytest.skip("needs two GPUs")
    e = entries_of(np.arange(100, dtype=np.int32), 1)
    a, b = bh.BloomFilter(1000, device=0), bh.BloomFilter(1000, device=1)
    a.set_batch_run(np.ascontiguousarray(e[:, 0]))
    b.set_batch_run(np.ascontiguousarray(e[:, 0]))
    with pytest.raises(bh.BloomHipError) as ei:
        bh.range_batch([a, b], [e, e], np.zeros(1, np.int32), np.ones(1, np.int32))
    assert ei.value.status == bh.EINVAL


@pytest.mark.parametrize("name", ["test-4", "test-5", "test-6"])
def test_reference_replay(name):
    """The recorded reference tests with `r` ops: the puts before each `r`, in
    put order, split into sorted runs of at most 512 distinct keys (a later put
    of a key replaces the value), the remainder the buffer, passed as runs[0]
    with no handle; filters sized as Run::Run does for 512 entries at the
    default 0.5 bits per entry.  The answer printed as the reference prints it
    equals the recorded stdout line of that op."""
    with open(os.path.join(ROOT, "tests", "golden", "ref_tests.json")) as fh:
        t = json.load(fh)["tests"][name]
    lines = t["expected_stdout"].split("\n")
    m = bh.m_bits(512, 0.5)
    assert m == 256
    flushed, buf, line, replayed = [], {}, 0, 0
    for op in t["ops"]:
        if op[0] == "p":
            if op[1] not in buf and len(buf) == 512:
                flushed.append(np.array(sorted(buf.items()), dtype=np.int32).reshape(-1, 2))
                buf = {}
            buf[op[1]] = op[2]
        elif op[0] == "g":
            line += 1
        elif op[0] == "r":
            ents = [np.array(sorted(buf.items()), dtype=np.int32).reshape(-1, 2)] + flushed[::-1]
            runs = [None] + [handle_for_m(e, m) for e in flushed[::-1]]
            off, out = bh.range_batch(runs, ents, np.array([op[1]], np.int32), np.array([op[2]], np.int32))
            got = " ".join(f"{k}:{v}" for k, v in out.tolist())
            assert got == lines[line].rstrip(), (op, got[:80], lines[line][:80])
            line += 1
            replayed += 1
    assert replayed == {"test-4": 1, "test-5": 1, "test-6": 3}[name]


def handle_for_m(e, m):
    f = bh.BloomFilter(m)
    f.set_batch_run(np.ascontiguousarray(e[:, 0]))
    return f


def test_fences_beyond_the_lds_budget():
    """One run of 15,361 * 4096 + 1 entries (15,362 fences: 61,448 bytes, past
    the 60 KiB of fences staged in LDS), made on the device: the page search
    reads the fences from global memory.  Arithmetic keys 68 * i - 2^31,
    values i: [s, e) answers i from ceil((s + 2^31) / 68) up to
    ceil((e + 2^31) / 68), clipped to the run."""
    torch = pytest.importorskip("torch")
    ne = 15_361 * 4096 + 1
    idx = torch.arange(ne, dtype=torch.int64, device="cuda")
    ent = torch.stack([(68 * idx - 2**31).to(torch.int32), idx.to(torch.int32)], dim=1).contiguous()
    del idx
    f = bh.BloomFilter(bh.m_bits(ne, 1.0))
    f.set_batch_run(ent.view(-1), n=ne, stride=8)
    fences, mk = f.run_meta()
    assert fences.size == 15_362 and fences.size * 4 > 60 << 10 and mk == 68 * (ne - 1) - 2**31
    rng = np.random.default_rng(8)
    edge = 68 * 4096 * rng.integers(1, 15_362, size=100) - 2**31     # interval edges
    s = np.concatenate([edge - 68 * 3, edge - 1, [68 * 1000 - 2**31 + 5, mk - 68 * 50_000 + 3]])
    e = np.concatenate([edge + 68 * 2 + 1, edge + 68 * 4, [68 * 4000 - 2**31 + 5, I32_MAX]])
    assert s.size == 202
    i0 = np.minimum(-((-(s + 2**31)) // 68), ne)
    i1 = np.maximum(np.minimum(-((-(e + 2**31)) // 68), ne), i0)
    cnt = i1 - i0
    assert cnt[:100].tolist() == [6] * 100 and cnt[200] == 3000 and cnt[201] > 40_000
    torch.cuda.synchronize()
    off, out = bh.range_batch([f], [ent], s.astype(np.int32), e.astype(np.int32))
    want_off = np.zeros(203, dtype=np.uint64)
    want_off[1:] = np.cumsum(cnt)
    assert np.array_equal(off, want_off)
    want_i = np.concatenate([np.arange(a, b) for a, b in zip(i0, i1)])
    assert np.array_equal(out[:, 1], want_i.astype(np.int32))
    assert np.array_equal(out[:, 0].astype(np.int64), 68 * want_i - 2**31)
