"""The numpy model of the compaction kernels (tests/merge_model.py), checked
without a GPU:

* its compaction equals the C oracle's MergeContext restatement (bo_compact)
  on random runs with repeated keys, so the (key, run, index) order it ranks
  samples by is the order the product has to keep;
* every input that tests/test_gpu_compact_edges.py runs has the property its
  case is there for: the partition counts, the fullest partition's size, the
  empty shares, the partitions that keep nothing.
"""
import numpy as np
import pytest

import merge_model as mm


@pytest.mark.parametrize("sizes,key_range", [([1], 5), ([700, 3, 900], 40), ([300] * 8, 500),
                                             ([5000, 1, 257, 256], 2000), ([2000] * 12, 3000)])
@pytest.mark.parametrize("drop", [False, True])
def test_model_compaction_is_the_oracles(coracle, sizes, key_range, drop):
    runs = mm.shared_key_runs(sizes, 17 * len(sizes) + key_range, key_range=key_range, repeats=True)
    assert np.array_equal(mm.compact(runs, drop), coracle.compact(runs, drop))


def test_model_merge_and_dedup_compose_to_the_compaction(coracle):
    # the pairwise path: a left fold of stable merges (newer on the left),
    # then the dedup
    runs = mm.shared_key_runs([900, 1, 2049, 300, 77], 5, key_range=700, repeats=True)
    merged = runs[0]
    for r in runs[1:]:
        merged = mm.merge2(merged, r)
    for drop in (False, True):
        assert np.array_equal(mm.dedup(merged, drop), coracle.compact(runs, drop))


def test_partition_bound_is_below_the_buffer():
    for k in range(1, mm.MAX_RUNS + 1):
        assert mm.max_partition(k) <= (mm.q_of(k) + k) * mm.S - 1 <= mm.CAP
    assert mm.max_partition(1) == 7936 and mm.max_partition(8) == 7929


@pytest.mark.parametrize("sizes", mm.RUN_LENGTHS, ids=lambda s: "-".join(map(str, s)))
def test_run_length_cases(sizes):
    runs = mm.run_length_case(sizes)
    assert [r.shape[0] for r in runs] == sizes
    st = mm.kway_stats(runs, False)
    # 1..256 entries are one sample, 257..512 two, 513 three; one partition
    want = {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 511: 2, 512: 2, 513: 3}
    assert [mm.nsamples(n) for n in sizes] == [want[n] for n in sizes]
    assert st["nparts"] == mm.kway_parts(sizes) == 1
    # keys are shared between the runs (or the run is alone)
    assert len(runs) == 1 or mm.compact(runs, False).shape[0] < sum(sizes)


@pytest.mark.parametrize("which", mm.SAMPLE_COUNTS)
@pytest.mark.parametrize("k", mm.SAMPLE_KS)
def test_sample_count_cases(k, which):
    runs = mm.sample_count_case(k, which)
    sizes = [r.shape[0] for r in runs]
    q = mm.q_of(k)
    assert sum(mm.nsamples(n) for n in sizes) == mm.sample_count_of(k, which)
    st = mm.kway_stats(runs, True)
    want = {"q-1": 1, "q": 1, "q+1": 2, "2q": 2, "2q+1": 3}[which]
    assert st["nparts"] == mm.kway_parts(sizes) == want
    assert st["sizes"].max() <= mm.max_partition(k)
    if which in ("q+1", "2q+1"):  # the last partition starts at the last-ranked sample
        assert 1 <= st["sizes"][-1] <= mm.S + (k - 1) * (mm.S - 1)


@pytest.mark.parametrize("a_newest", [True, False], ids=["a_newest", "a_oldest"])
@pytest.mark.parametrize("k", range(1, mm.MAX_RUNS + 1))
def test_fullest_partition_cases(k, a_newest):
    runs = mm.fullest_partition_case(k, a_newest)
    assert sum(r.shape[0] for r in runs) < 25_000
    q = mm.q_of(k)
    st = mm.kway_stats(runs, True)
    assert st["sizes"][1] == mm.max_partition(k) == q * 256 + (k - 1) * 255
    assert st["sizes"].max() == st["sizes"][1] <= mm.CAP
    ra = 0 if a_newest else k - 1
    for r in range(k):
        assert st["shares"][1, r] == (q * 256 if r == ra else 255)
    # every inside key is one of A's: the dedup drops one copy of each, and
    # which copy stays flips with A's age
    total = sum(r.shape[0] for r in runs)
    out = mm.compact(runs, False)
    assert total - out.shape[0] >= 1 or k == 1
    inside = out[(out[:, 0] >= 0) & (out[:, 0] < runs[ra].shape[0])]
    assert inside.shape[0] == runs[ra].shape[0]
    winners = np.where(inside[:, 1] == mm.TOMB, -1, inside[:, 1].astype(np.int64) >> 24)
    live = winners[winners >= 0]
    if a_newest:
        assert (live == 0).all()
    elif k > 1:
        assert (live != ra).any() and (live == ra).any()


@pytest.mark.parametrize("tomb", [False, True], ids=["live", "tombstone"])
@pytest.mark.parametrize("key", mm.EQUAL_KEYS)
def test_equal_key_cases(key, tomb):
    runs = mm.equal_keys_case(key, tomb)
    st = mm.kway_stats(runs, True)
    assert st["nparts"] == 2
    # partition 1 starts inside run 2's equal keys, every run has entries before it
    assert list(st["bounds"][1]) == [600, 300, (mm.q_of(3) - 5) * 256]
    assert list(st["kept"]) == [0 if tomb else 1, 0]
    assert mm.compact(runs, True).shape[0] == (0 if tomb else 1)
    assert mm.compact(runs, False).shape[0] == 1


def test_tombstone_stretch_case():
    runs = mm.tombstone_stretch_case()
    assert 39_000 <= sum(r.shape[0] for r in runs) <= 41_000
    kept = mm.kway_stats(runs, True)["kept"]
    zeros = np.flatnonzero(kept == 0)
    assert zeros.size >= 2 and (np.diff(zeros) == 1).all()  # one stretch of empty partitions
    assert kept[:zeros[0]].sum() > 0 and kept[zeros[-1] + 1:].sum() > 0
    assert kept[zeros[0] - 1] > 0 and kept[zeros[-1] + 1] > 0


@pytest.mark.parametrize("descending", [True, False], ids=["descending", "ascending"])
@pytest.mark.parametrize("n", [5000, 8000])
def test_disjoint_cases(n, descending):
    runs = mm.disjoint_case(n, descending)
    for r in range(3):
        lo, hi = (runs[r + 1], runs[r]) if descending else (runs[r], runs[r + 1])
        assert lo[-1, 0] < hi[0, 0]
    shares = mm.kway_stats(runs, True)["shares"]
    empty = (shares == 0).sum(axis=1)
    # a partition is q = 28 samples, 7,168 entries: at 5,000 entries a run it
    # spans two runs (two shares empty), at 8,000 some lie inside one run
    assert (empty >= 2).all()
    if n == 8000:
        assert (empty == 3).sum() >= 2


@pytest.mark.parametrize("pattern", mm.PAIR_PATTERNS)
@pytest.mark.parametrize("na,nb", mm.PAIR_SIZES)
def test_pair_cases(na, nb, pattern):
    a, b = mm.pair_case(na, nb, pattern)
    assert (a.shape[0], b.shape[0]) == (na, nb)
    out = mm.merge2(a, b)
    assert (np.diff(out[:, 0].astype(np.int64)) >= 0).all()
    src = out[:, 1] >> 24
    if pattern == "a_first" or pattern == "equal":
        assert (np.diff(src) >= 0).all()  # all of a, then all of b
    if pattern == "b_first" and na and nb:
        assert src[0] == 1 and src[-1] == 0
    if pattern == "ties" and na > 1000 and nb > 1000:  # a key in both inputs: a's copies first
        both = np.intersect1d(a[:, 0], b[:, 0])
        assert both.size
        sel = src[out[:, 0] == both[0]]
        assert (np.diff(sel) >= 0).all() and sel[0] == 0 and sel[-1] == 1


def test_round_cases():
    for npairs, empty_at in [(2, None), (7, None), (8, None), (7, 3), (8, 7)]:
        pairs = mm.round_case(npairs, empty_at)
        assert len(pairs) == npairs <= mm.MAX_PAIRS
        sizes = [a.shape[0] + b.shape[0] for a, b in pairs]
        if empty_at is not None:
            assert sizes[empty_at] == 0 and sum(1 for s in sizes if s == 0) == 1
        assert len({-(-s // mm.MERGE_TILE) for s in sizes}) >= 2  # pairs of 1 and of more tiles
    assert mm.MAX_PAIRS == 8


@pytest.mark.parametrize("pattern", mm.DEDUP_PATTERNS)
@pytest.mark.parametrize("n", mm.DEDUP_SIZES)
def test_dedup_cases(n, pattern):
    e = mm.dedup_case(n, pattern)
    assert e.shape[0] == n
    keys = e[:, 0]
    if pattern.startswith("twice") and n > 4097:
        eq = np.flatnonzero(keys[1:] == keys[:-1])  # pairs (i, i + 1)
        par = 0 if pattern == "twice_from_0" else 1
        assert (eq % 2 == par).all()
        # from 1: a pair across two vectors, two 512-entry rounds and two tiles
        if par:
            assert 511 in eq and 4095 in eq
        else:
            assert 510 in eq and 4094 in eq
    want = {"distinct": n, "equal": 1}.get(pattern)
    if want:
        assert mm.dedup(e, False).shape[0] == want


@pytest.mark.parametrize("nruns", mm.MANY_RUNS)
def test_many_runs_cases(nruns):
    runs = mm.many_runs_case(nruns)
    assert len(runs) == nruns > mm.MAX_RUNS
    total = sum(r.shape[0] for r in runs)
    assert mm.compact(runs, False).shape[0] < total / 2 or nruns < 11  # most keys in several runs
    # the merge tree: rounds with an odd run to copy, and their pair counts
    n, pairs, odd = nruns, [], []
    while n > 1:
        pairs.append(n // 2)
        odd.append(n % 2)
        n = (n + 1) // 2
    want = {9: ([4, 2, 1, 1], 3), 10: ([5, 2, 1, 1], 2), 11: ([5, 3, 1, 1], 2), 16: ([8, 4, 2, 1], 0),
            17: ([8, 4, 2, 1, 1], 4), 18: ([9, 4, 2, 1, 1], 3), 33: ([16, 8, 4, 2, 1, 1], 5),
            64: ([32, 16, 8, 4, 2, 1], 0)}[nruns]
    assert (pairs, sum(odd)) == want


def test_second_chunk_runs_reach_the_second_chunk():
    sizes = [466_490] * 9
    total = sum(sizes)
    assert total > 4_198_400 and -(-total // mm.DEDUP_TILE) > mm.SCAN_CHUNK + 1
    # (the arrays themselves are built, and compared with the oracle, on the GPU test)
