"""GPU parity of the batched GET (bloomhip_get_batch): routing, then the
candidate runs read on the device until one holds the key
(LSMTree::get past the buffer, src/lsm_tree.cpp:173-215; Run::get,
src/run.cpp:85-113, over the fence interval the fences describe).

Expected answers come from a numpy model: found_run is the first run, in
order, whose key array contains the key, vals that entry's value; stats
follow from the C oracle's candidate rows (coracle.route): a run's page is
read for a key when the run is a candidate and no newer run held the key.
Everything is compared exactly."""
import ctypes
import json
import os

import numpy as np
import pytest

import bloomhip as bh
from test_gpu_route import sorted_run

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2**31, 2**31 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def entries_of(keys, seed):
    """entry_t records of a run: the keys with seeded values (no tombstones)."""
    rng = np.random.default_rng(seed)
    e = np.empty((keys.size, 2), dtype=np.int32)
    e[:, 0] = keys
    e[:, 1] = rng.integers(I32_MIN + 1, 2**31, size=keys.size, dtype=np.int64).astype(np.int32)
    return e


def build(coracle, spec):
    """spec: [(entries, m, meta)] newest first -> (handles, oracle refs);
    meta=False: a filter with no run metadata (never a candidate)."""
    runs, orefs = [], []
    for e, m, meta in spec:
        keys = np.ascontiguousarray(e[:, 0])
        f = bh.BloomFilter(m)
        if meta:
            f.set_batch_run(keys)
            fences, mk = coracle.run_meta(keys)
        else:
            f.set_batch(keys)
            fences, mk = np.zeros(0, np.int32), 0
        runs.append(f)
        orefs.append((coracle.build(m, keys), m, fences, mk))
    return runs, orefs


def model(coracle, spec, orefs, gets):
    """(vals, found_run, stats) the call must return."""
    n = gets.size
    found = np.full(n, -1, dtype=np.int32)
    vals = np.full(n, I32_MIN, dtype=np.int32)
    for r, (e, _, _) in enumerate(spec):
        if e.shape[0] == 0:
            continue
        idx = np.minimum(np.searchsorted(e[:, 0], gets), e.shape[0] - 1)
        hit = (e[idx, 0] == gets) & (found < 0)
        found[hit] = r
        vals[hit] = e[idx[hit], 1]
    stats = np.zeros((len(spec), 2), dtype=np.uint64)
    if n:
        cand, _, _ = coracle.route(orefs, gets)
        for r in range(len(spec)):
            c = np.unpackbits(cand[r].view(np.uint8), bitorder="little")[:n].astype(bool)
            visited = int((c & ((found < 0) | (found >= r))).sum())
            stats[r, 0] = visited
            stats[r, 1] = visited - int((found == r).sum())
    return vals, found, stats


def check(coracle, spec, gets, runs=None, orefs=None, **kw):
    if runs is None:
        runs, orefs = build(coracle, spec)
    want = model(coracle, spec, orefs, gets)
    vals, found, stats = bh.get_batch(runs, [e for e, _, _ in spec], gets, **kw)
    assert np.array_equal(found, want[1])
    assert np.array_equal(vals, want[0])
    assert np.array_equal(stats, want[2]), (stats, want[2])
    return want


def edge_gets(spec, extra=()):
    """Every run's first and last key, the first and last key of every fence
    interval and their +-1 neighbours, both int32 extremes, and duplicates."""
    ks = [np.array([I32_MIN, I32_MAX], dtype=np.int64)]
    for e, _, _ in spec:
        k = e[:, 0].astype(np.int64)
        if k.size == 0:
            continue
        starts = k[::4096]
        ends = np.concatenate([k[4095::4096], k[-1:]])
        b = np.concatenate([k[:1], k[-1:], starts, ends])
        ks.append(np.concatenate([b - 1, b, b + 1]))
    ks.extend(np.asarray(x, dtype=np.int64) for x in extra)
    g = np.clip(np.concatenate(ks), I32_MIN, I32_MAX).astype(np.int32)
    return np.concatenate([g, np.repeat(g[2:3], 70)])  # one key many times


RUN_SIZES = [0, 1, 511, 512, 513, 4095, 4096, 4097, 12_289]


@pytest.fixture(scope="module")
def sized(coracle):
    """One run of every size of RUN_SIZES (the empty one without metadata),
    built once and left unchanged."""
    spec = []
    for j, n in enumerate(RUN_SIZES):
        keys = sorted_run(n, 300 + j)
        spec.append((entries_of(keys, 400 + j), bh.m_bits(max(n, 1), 10.0), n > 0))
    runs, orefs = build(coracle, spec)
    return spec, runs, orefs


def test_run_sizes_and_interval_edges(coracle, sized):
    spec, runs, orefs = sized
    rng = np.random.default_rng(1)
    pool = np.concatenate([e[:, 0] for e, _, _ in spec])
    gets = np.concatenate([edge_gets(spec), pool[rng.integers(0, pool.size, size=3000)],
                           rng.integers(I32_MIN, 2**31, size=1000, dtype=np.int64).astype(np.int32)])
    vals, found, stats = check(coracle, spec, gets, runs, orefs)
    assert set(np.unique(found)) == set(range(1, len(spec))) | {-1}  # every non-empty run answers
    assert stats[0, 0] == 0 and stats[:, 1].sum() > 0
    # each size alone, with its own edges
    for j in range(len(spec)):
        check(coracle, spec[j:j + 1], edge_gets(spec[j:j + 1]), runs[j:j + 1], orefs[j:j + 1])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 10_000])
def test_get_counts(coracle, sized, n):
    spec, runs, orefs = sized
    rng = np.random.default_rng(n)
    pool = np.concatenate([e[:, 0] for e, _, _ in spec])
    gets = np.concatenate([pool[rng.integers(0, pool.size, size=n // 2)],
                           rng.integers(I32_MIN, 2**31, size=n - n // 2, dtype=np.int64).astype(np.int32)])
    rng.shuffle(gets)
    if n == 0:
        # stats are overwritten with zeros even when there is nothing to do
        stats = np.full((len(runs), 2), 7, dtype=np.uint64)
        v, f, s = bh.get_batch(runs, [e for e, _, _ in spec], gets, vals=np.empty(0, np.int32),
                               found_run=np.empty(0, np.int32), stats=stats)
        assert not s.any()
        return
    check(coracle, spec, gets, runs, orefs)


@pytest.mark.parametrize("nruns", [1, 2, 5, 16, 17, 64])
def test_run_counts(coracle, nruns):
    small = nruns > 16
    spec = []
    for j in range(nruns):
        n = 300 + 7 * j if small else [4097, 600, 9000, 513, 5000][j % 5]
        # a narrow key range, so that runs overlap and false positives happen
        rng = np.random.default_rng(50 + j)
        keys = np.unique(rng.integers(-20_000, 20_000, size=n, dtype=np.int64).astype(np.int32))
        spec.append((entries_of(keys, 60 + j), bh.m_bits(keys.size, 3.0), True))
    gets = np.concatenate([np.arange(-20_010, 20_010, 7, dtype=np.int32), edge_gets(spec)])
    vals, found, stats = check(coracle, spec, gets)
    assert (found == nruns - 1).any() and stats[:, 1].sum() > 100


def test_newest_wins_and_tombstones(coracle):
    keys = np.arange(0, 6000, 3, dtype=np.int32)
    spec = []
    for j in range(3):
        e = entries_of(keys, 70 + j)
        e[:, 1] = 1000 * (j + 1) + (np.arange(keys.size) % 1000)
        spec.append((e, bh.m_bits(keys.size, 10.0), True))
    # a tombstone in the newest run over live values in the older ones, and
    # one in the middle run under a live value
    spec[0][0][5, 1] = I32_MIN
    spec[1][0][9, 1] = I32_MIN
    only_old = np.arange(1, 6000, 3, dtype=np.int32)[:500]   # keys of the oldest run alone
    e3 = entries_of(only_old, 75)
    e3[7, 1] = I32_MIN
    spec.append((e3, bh.m_bits(only_old.size, 10.0), True))
    gets = np.concatenate([keys, only_old, np.arange(2, 600, 3, dtype=np.int32)])
    vals, found, stats = check(coracle, spec, gets)
    assert (found[:keys.size] == 0).all()                     # one key, three values: the newest
    assert (vals[:keys.size] == spec[0][0][:, 1]).all()
    assert vals[5] == I32_MIN and found[5] == 0               # tombstone hides the older values
    assert vals[9] == spec[0][0][9, 1]
    assert found[keys.size + 7] == 3 and vals[keys.size + 7] == I32_MIN
    assert (found[keys.size + only_old.size:] == -1).all()


def test_fall_through_on_false_positives(coracle):
    """Filters at 1 bit per key: most reads are false positives and the GET
    must go on to older runs; then a 1-bit filter, where every key in range
    is a candidate."""
    sizes = [513, 4097, 12_289]
    spec = []
    for j, n in enumerate(sizes):
        keys = sorted_run(n, 100 + j)
        spec.append((entries_of(keys, 80 + j), bh.m_bits(n, 1.0), True))
    rng = np.random.default_rng(9)
    pool = np.concatenate([e[:, 0] for e, _, _ in spec])
    gets = np.concatenate([pool[rng.integers(0, pool.size, size=5000)],
                           rng.integers(I32_MIN, 2**31, size=5000, dtype=np.int64).astype(np.int32)])
    runs, orefs = build(coracle, spec)
    want_vals, want_found, want_stats = model(coracle, spec, orefs, gets)
    _, wf, _ = coracle.route(orefs, gets)
    fell = int(((wf >= 0) & (want_found > wf)).sum())  # answered by a run older than the first candidate
    print("fall-through GETs", fell, "false reads per run", want_stats[:, 1].tolist())
    assert fell >= 1000, fell          # a vacuous input must not pass
    assert (want_stats[:, 1] > 1000).all()
    check(coracle, spec, gets, runs, orefs)
    one_bit = [(e, 1, True) for e, _, _ in spec]
    vals, found, stats = check(coracle, one_bit, gets)
    assert stats[0, 0] >= ((gets >= spec[0][0][0, 0]) & (gets <= spec[0][0][-1, 0])).sum()


@pytest.mark.parametrize("search", ["binary", "interp"])
def test_adversarial_key_distributions(coracle, search, monkeypatch):
    """Consecutive integers, and half the keys within 10,000 of INT32_MIN and
    half within 10,000 of INT32_MAX: interpolation guesses are exact in the
    first and useless in the second; both forms of the interval search must
    be exact.  GETs: all stored keys plus the gaps."""
    monkeypatch.setenv("BLOOMHIP_GET_SEARCH", search)
    rng = np.random.default_rng(3)
    consecutive = np.arange(-6000, -6000 + 12_289, dtype=np.int32)
    lo = I32_MIN + np.sort(rng.choice(10_000, size=6144, replace=False))
    hi = I32_MAX - 10_000 + np.sort(rng.choice(10_000, size=6145, replace=False))
    split = np.concatenate([lo, hi]).astype(np.int32)
    # a dense cluster plus a sparse tail inside single intervals
    skew = np.unique(np.concatenate([rng.integers(0, 30_000, size=11_000, dtype=np.int64),
                                     rng.integers(I32_MIN, 2**31, size=1289, dtype=np.int64)])).astype(np.int32)
    for keys in (consecutive, split, skew):
        spec = [(entries_of(keys, 90), bh.m_bits(keys.size, 10.0), True)]
        k64 = keys.astype(np.int64)
        gaps = np.concatenate([np.arange(I32_MIN, I32_MIN + 10_001), np.arange(I32_MAX - 10_001, I32_MAX + 1),
                               np.arange(-6100, 6400), np.arange(-100, 30_100, 3), k64 - 1, k64 + 1])
        gets = np.clip(np.concatenate([k64, gaps]), I32_MIN, I32_MAX).astype(np.int32)
        vals, found, stats = check(coracle, spec, gets)
        assert (found[:keys.size] == 0).all() and (found == -1).any()


@pytest.mark.parametrize("search", ["binary", "interp"])
def test_both_search_forms_on_uniform_runs(coracle, sized, search, monkeypatch):
    monkeypatch.setenv("BLOOMHIP_GET_SEARCH", search)
    spec, runs, orefs = sized
    rng = np.random.default_rng(4)
    pool = np.concatenate([e[:, 0] for e, _, _ in spec])
    gets = np.concatenate([edge_gets(spec), pool[rng.integers(0, pool.size, size=5000)]])
    check(coracle, spec, gets, runs, orefs)


@pytest.mark.parametrize("stride", [4, 8, 12])
def test_key_strides(coracle, sized, stride):
    spec, runs, orefs = sized
    gets = edge_gets(spec)
    buf = np.zeros((gets.size, stride // 4), dtype=np.int32)
    buf[:, 0] = gets
    want = model(coracle, spec, orefs, gets)
    vals, found, stats = bh.get_batch(runs, [e for e, _, _ in spec], buf.reshape(-1), n=gets.size,
                                      stride=stride)
    assert np.array_equal(vals, want[0]) and np.array_equal(found, want[1])
    assert np.array_equal(stats, want[2])


@pytest.mark.parametrize("keys_dev", [False, True], ids=["hostkeys", "devkeys"])
@pytest.mark.parametrize("ent_dev", [False, True], ids=["hostent", "devent"])
@pytest.mark.parametrize("out_dev", [False, True], ids=["hostout", "devout"])
def test_residency(coracle, sized, keys_dev, ent_dev, out_dev):
    torch = pytest.importorskip("torch")
    spec, runs, orefs = sized
    gets = edge_gets(spec)
    n = gets.size
    want = model(coracle, spec, orefs, gets)
    k = torch.from_numpy(gets).cuda() if keys_dev else gets
    ents = [torch.from_numpy(e).cuda() if ent_dev else e for e, _, _ in spec]
    stream = runs[0].stream_ptr() if (keys_dev and ent_dev and out_dev) else None
    if stream is not None:
        torch.cuda.synchronize()  # the uploads above ran on torch's stream
    if out_dev:
        dv = torch.empty(n, dtype=torch.int32, device="cuda")
        df = torch.empty(n, dtype=torch.int32, device="cuda")
        ds = torch.full((len(runs), 2), 5, dtype=torch.int64, device="cuda")
        bh.get_batch(runs, ents, k, vals=dv, found_run=df, stats=ds, stream=stream)
        runs[0].sync(stream)
        torch.cuda.synchronize()
        vals, found = dv.cpu().numpy(), df.cpu().numpy()
        stats = ds.cpu().numpy().view(np.uint64)
    else:
        vals, found, stats = bh.get_batch(runs, ents, k)
    assert np.array_equal(vals, want[0]) and np.array_equal(found, want[1])
    assert np.array_equal(stats, want[2])


def test_optional_outputs(coracle, sized):
    spec, runs, orefs = sized
    gets = edge_gets(spec)
    want = model(coracle, spec, orefs, gets)
    ents = [e for e, _, _ in spec]
    n = gets.size
    v, f, s = bh.get_batch(runs, ents, gets, vals=np.empty(n, np.int32))
    assert f is None and s is None and np.array_equal(v, want[0])
    v, f, s = bh.get_batch(runs, ents, gets, found_run=np.empty(n, np.int32))
    assert v is None and s is None and np.array_equal(f, want[1])
    v, f, s = bh.get_batch(runs, ents, gets, stats=np.full((len(runs), 2), 9, np.uint64))
    assert v is None and f is None and np.array_equal(s, want[2])


def test_fences_beyond_the_lds_budget(coracle):
    """One run of 15,361 * 4096 + 1 entries (15,362 fences: 61,448 bytes, past
    the 60 KiB of fences staged in LDS), made on the device: the page search
    reads the fences from global memory.  Arithmetic keys 68 * i - 2^31 (all
    of int32), values i; filter at 1 bit per key."""
    torch = pytest.importorskip("torch")
    ne = 15_361 * 4096 + 1
    idx = torch.arange(ne, dtype=torch.int64, device="cuda")
    ent = torch.stack([(68 * idx - 2**31).to(torch.int32), idx.to(torch.int32)], dim=1).contiguous()
    del idx
    m = bh.m_bits(ne, 1.0)
    f = bh.BloomFilter(m)
    f.set_batch_run(ent.view(-1), n=ne, stride=8)
    keys = ent[:, 0].contiguous().cpu().numpy()
    fences, mk = coracle.run_meta(keys)
    assert fences.size == 15_362 and fences.size * 4 > 60 << 10 and mk == 68 * (ne - 1) - 2**31
    oref = [(coracle.build_mt(m, keys, 8), m, fences, mk)]
    rng = np.random.default_rng(8)
    fstart = 68 * 4096 * rng.integers(0, 15_362, size=2000) - 2**31    # interval edges
    gets = np.concatenate([
        [I32_MIN, I32_MIN + 1, mk, mk - 1, mk + 1, I32_MAX], fstart, fstart - 68, fstart + 68,
        68 * rng.integers(0, ne, size=46_994) - 2**31,                  # stored keys
        rng.integers(I32_MIN, 2**31, size=47_000, dtype=np.int64)])
    gets = np.clip(gets, I32_MIN, I32_MAX)
    assert gets.size == 100_000
    q, rem = np.divmod(gets + 2**31, 68)
    there = (rem == 0) & (q < ne)
    cand, _, _ = coracle.route(oref, gets.astype(np.int32))
    c = np.unpackbits(cand[0].view(np.uint8), bitorder="little")[:gets.size].astype(bool)
    assert (c | ~there).all()  # no false negatives in the oracle's rows
    vals, found, stats = bh.get_batch([f], [ent], gets.astype(np.int32))
    assert np.array_equal(found, np.where(there, 0, -1))
    assert np.array_equal(vals, np.where(there, q, I32_MIN).astype(np.int32))
    assert stats.tolist() == [[int(c.sum()), int(c.sum()) - int(there.sum())]]
    assert there.sum() > 40_000 and (c & ~there).sum() > 10_000


def test_argument_errors():
    L = bh.lib()
    keys = np.arange(100, dtype=np.int32)
    e = entries_of(np.arange(5000, dtype=np.int32), 1)
    f = bh.BloomFilter(1000)
    f.set_batch_run(np.ascontiguousarray(e[:, 0]))  # 2 fences
    f.profile(True)
    f.profile_reset()
    vals = np.full(100, 77, dtype=np.int32)

    def call(handles, eptrs, sizes, nruns):
        H = (ctypes.c_void_p * 80)(*handles)
        E = (ctypes.c_void_p * 80)(*eptrs)
        N = (ctypes.c_size_t * 80)(*sizes)
        return L.bloomhip_get_batch(H, E, N, nruns, 0, keys.ctypes.data, keys.size, 4, 0,
                                    vals.ctypes.data, None, None, 0, None)

    h, p = f.handle.value, e.ctypes.data
    assert call([h], [p], [5000], 1) == bh.OK
    vals[:] = 77
    f.profile_reset()
    assert call([h], [p], [4096], 1) == bh.EINVAL        # 2 fences, entries for 1
    assert call([h], [p], [8193], 1) == bh.EINVAL        # entries for 3
    assert call([h], [None], [5000], 1) == bh.EINVAL     # NULL entries, nentries > 0
    assert call([h], [p], [5000], 0) == bh.EINVAL
    assert call([h] * 65, [p] * 65, [5000] * 65, 65) == bh.EINVAL
    if bh.device_count() > 1:
        g = bh.BloomFilter(1000, device=1)
        assert call([h, g.handle.value], [p, None], [5000, 0], 2) == bh.EINVAL
    assert (vals == 77).all() and f.profile_read() == {}  # nothing was launched
    f.profile(False)


def test_runs_on_two_devices_refused():
    if bh.device_count() < 2:
        pytest.skip("needs two GPUs")
    e = entries_of(np.arange(100, dtype=np.int32), 1)
    a, b = bh.BloomFilter(1000, device=0), bh.BloomFilter(1000, device=1)
    a.set_batch_run(np.ascontiguousarray(e[:, 0]))
    b.set_batch_run(np.ascontiguousarray(e[:, 0]))
    with pytest.raises(bh.BloomHipError) as ei:
        bh.get_batch([a, b], [e, e], np.arange(10, dtype=np.int32))
    assert ei.value.status == bh.EINVAL


def test_reference_test6_replayed():
    """tests/golden/ref_tests.json test-6: the puts `p k k` flush as three
    512-entry runs at bits_per_entry 0.5 (m = 256); every key answers with its
    own value from its own run, `g 1535` with 1535 (the recorded stdout's
    second line).  Runs of 512 entries: the reference's 512-entry page window
    and the fence interval agree."""
    with open(os.path.join(ROOT, "tests", "golden", "ref_tests.json")) as fh:
        t = json.load(fh)["tests"]["test-6"]
    puts = [op for op in t["ops"] if op[0] == "p"][:1536]
    flushed = [np.array([[k, v] for _, k, v in puts[i:i + 512]], dtype=np.int32)
               for i in range(0, 1536, 512)]
    ents = [np.ascontiguousarray(e[np.argsort(e[:, 0], kind="stable")]) for e in flushed[::-1]]  # newest first
    m = bh.m_bits(512, 0.5)
    assert m == 256
    runs = []
    for e in ents:
        f = bh.BloomFilter(m)
        f.set_batch_run(np.ascontiguousarray(e[:, 0]))
        runs.append(f)
    keys = np.arange(1536, dtype=np.int32)
    vals, found, stats = bh.get_batch(runs, ents, keys)
    assert np.array_equal(vals, keys)
    assert np.array_equal(found, 2 - keys // 512)
    assert ["g", 1535] in t["ops"] and t["expected_stdout"].splitlines()[1] == "1535"
    assert vals[1535] == 1535
    assert stats[:, 0].sum() - stats[:, 1].sum() == 1536


def test_profile_slot(coracle, sized):
    spec, runs, orefs = sized
    gets = edge_gets(spec)
    f0 = runs[0]
    f0.profile(True)
    f0.profile_reset()
    try:
        bh.get_batch(runs, [e for e, _, _ in spec], gets)
        bh.get_batch(runs, [e for e, _, _ in spec], gets)
        prof = f0.profile_read()
    finally:
        f0.profile(False)
    assert prof["k_get_resolve"]["launches"] == 2
    assert bh.PROF_SLOTS == 13
