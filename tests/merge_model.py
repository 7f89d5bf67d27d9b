"""A plain numpy model of the compaction kernels (csrc/bloom_merge.hip), shared
by tests/test_merge_model_host.py and tests/test_gpu_compact_edges.py.

Runs are int32 [n, 2] arrays of (key, value), key-sorted, newest first.  The
total order of all entries is (key, run, index): among equal keys the newest
run's first entry comes first, and the compaction keeps the first entry of
every key (not a tombstone when they are dropped).

* the one-pass k-way kernels' partitioner: every S-th entry of every run is a
  sample; the samples are ranked in the total order; every rank that is a
  non-zero multiple of q = 32 - k starts a partition; the start's position in a
  run is the number of that run's entries before the sample (x, r) -- key < x,
  or key == x in a newer run -- and j * S in the sample's own run;
* the stable two-way merge of the pairwise rounds (the left input wins ties);
* the dedup pass (first entry of every key, tombstones dropped on request).

The second half builds the inputs of the edge cases; the host test proves each
one's property on the model, so the GPU test cannot miss its edge silently.
"""
import numpy as np

TOMB = -2**31        # VAL_TOMBSTONE
I32_MIN, I32_MAX = -2**31, 2**31 - 1
S = 256              # kKwayS: the sample stride
CAP = 32 * S         # kKwayCap: entries of one partition's LDS buffer
MAX_RUNS = 8         # kKwayMaxRuns
MERGE_TILE = 2048    # kMergeTile: outputs per workgroup of a merge round
MAX_PAIRS = 8        # kMaxMergePairs
DEDUP_TILE = 4096    # kCompactTile
SCAN_CHUNK = 1024    # tiles per step of k_scan_counts


def q_of(k):
    """Samples per partition at fan-in k."""
    return CAP // S - k


def nsamples(n):
    return -(-n // S)


def kway_parts(sizes):
    ns = sum(nsamples(n) for n in sizes)
    return (ns - 1) // q_of(len(sizes)) + 1 if ns else 0


def max_partition(k):
    """The most entries a partition can hold: 256 behind each of its q
    samples, and of every run but the one whose sample starts it the 255
    between that run's last sample before the start and the start."""
    return q_of(k) * S + (k - 1) * (S - 1)


def kway_bounds(runs):
    """The partition table: (nparts + 1, k) int64, row p column r = the first
    entry of run r in partition p; the last row holds the runs' lengths."""
    k = len(runs)
    q = q_of(k)
    keys = [r[:, 0].astype(np.int64) for r in runs]
    sk = np.concatenate([kk[::S] for kk in keys])
    sr = np.concatenate([np.full(nsamples(kk.size), r) for r, kk in enumerate(keys)])
    sj = np.concatenate([np.arange(nsamples(kk.size)) for kk in keys])
    order = np.lexsort((sj, sr, sk))  # rank -> sample, by (key, run, index)
    nparts = (sk.size - 1) // q + 1
    bounds = np.zeros((nparts + 1, k), dtype=np.int64)
    bounds[nparts] = [kk.size for kk in keys]
    for p in range(1, nparts):
        g = order[p * q]
        x, r, j = sk[g], sr[g], sj[g]
        for rr in range(k):
            if rr == r:
                bounds[p, rr] = j * S
            else:  # a newer run's entries of key x come before (x, r)
                bounds[p, rr] = np.searchsorted(keys[rr], x, "right" if rr < r else "left")
    return bounds


def total_order(runs):
    """All entries in (key, run, index) order: keys, values, runs, indices."""
    key = np.concatenate([r[:, 0] for r in runs]).astype(np.int64)
    val = np.concatenate([r[:, 1] for r in runs]).astype(np.int64)
    run = np.concatenate([np.full(r.shape[0], i) for i, r in enumerate(runs)])
    idx = np.concatenate([np.arange(r.shape[0]) for r in runs])
    o = np.lexsort((idx, run, key))
    return key[o], val[o], run[o], idx[o]


def keep_flags(key, val, drop):
    first = np.ones(key.size, dtype=bool)
    first[1:] = key[1:] != key[:-1]
    return first & ~(val == TOMB) if drop else first


def compact(runs, drop):
    """The compaction of the runs: int32 [n_out, 2]."""
    runs = [r for r in runs if r.shape[0]]
    if not runs:
        return np.empty((0, 2), dtype=np.int32)
    key, val, _, _ = total_order(runs)
    keep = keep_flags(key, val, drop)
    return np.stack([key[keep], val[keep]], axis=1).astype(np.int32)


def kway_stats(runs, drop):
    """What the one-pass kernels make of the runs: the bounds table, the
    shares (nparts, k), the partitions' sizes and their kept counts."""
    bounds = kway_bounds(runs)
    shares = np.diff(bounds, axis=0)
    assert (shares >= 0).all()
    key, val, run, idx = total_order(runs)
    part = np.empty(key.size, dtype=np.int64)
    for r in range(len(runs)):
        sel = run == r
        part[sel] = np.searchsorted(bounds[:, r], idx[sel], "right") - 1
    assert (np.diff(part) >= 0).all(), "partitions are ranges of the total order"
    nparts = bounds.shape[0] - 1
    kept = np.bincount(part[keep_flags(key, val, drop)], minlength=nparts)
    sizes = shares.sum(axis=1)
    assert np.array_equal(sizes, np.bincount(part, minlength=nparts))
    return dict(bounds=bounds, shares=shares, sizes=sizes, kept=kept, nparts=nparts)


def merge2(a, b):
    """Stable merge of two key-sorted entry arrays, a winning ties."""
    both = np.concatenate([a, b])
    return both[np.argsort(both[:, 0], kind="stable")]


def dedup(e, drop):
    """First entry of every key of a key-sorted entry array."""
    if e.shape[0] == 0:
        return e
    return e[keep_flags(e[:, 0].astype(np.int64), e[:, 1].astype(np.int64), drop)]


# --------------------------------------------------------------------------
# Constructed inputs.  Values encode run << 24 | index (tombstones aside), so a
# wrong winner among equal keys or a broken tie order shows in the output.
# --------------------------------------------------------------------------
def entries(keys, run, tomb=None):
    keys = np.asarray(keys, dtype=np.int64)
    vals = (run << 24) | np.arange(keys.size, dtype=np.int64)
    if tomb is not None:
        vals[np.asarray(tomb, dtype=bool)] = TOMB
    assert (np.diff(keys) >= 0).all()
    return np.ascontiguousarray(np.stack([keys, vals], axis=1).astype(np.int32))


def shared_key_runs(sizes, seed, key_range=None, repeats=False):
    """Runs of the given sizes whose keys come from one small range, so most
    keys are in several runs; about one entry in eight a tombstone."""
    rng = np.random.default_rng(seed)
    key_range = key_range or max(1, 3 * max(sizes) // 2)
    runs = []
    for r, n in enumerate(sizes):
        keys = np.sort(rng.integers(0, key_range, size=n) if repeats
                       else rng.choice(key_range, size=n, replace=False)) - key_range // 2
        runs.append(entries(keys, r, rng.random(n) < 0.125))
    return runs


# run lengths around the sample stride: how many samples a run has
RUN_LENGTHS = ([[n] for n in (1, 255, 256, 257, 511, 512, 513)] +
               [[1, 1], [1, 257], [256, 256], [257, 255], [513, 1]] +
               [[1] * 8, [257, 1, 256, 255, 513, 1, 512, 2]])


def run_length_case(sizes):
    return shared_key_runs(sizes, 1000 + sum(sizes) + len(sizes))


# total sample counts around the partition size: nparts = 1, 1, 2, 2, 3
SAMPLE_KS = (1, 2, 5, 8)
SAMPLE_COUNTS = ("q-1", "q", "q+1", "2q", "2q+1")


def sample_count_of(k, which):
    q = q_of(k)
    return {"q-1": q - 1, "q": q, "q+1": q + 1, "2q": 2 * q, "2q+1": 2 * q + 1}[which]


def sample_count_case(k, which):
    """k runs with sample_count_of(k, which) samples in all, the runs' last
    sample blocks of 1, 255, 256, 100, ... entries; repeated keys."""
    ns = sample_count_of(k, which)
    tails = (1, 255, 256, 100)
    sizes = []
    for r in range(k):
        c = ns // k + (1 if r < ns % k else 0)
        assert c >= 1
        sizes.append((c - 1) * S + tails[r % 4])
    assert sum(nsamples(n) for n in sizes) == ns
    return shared_key_runs(sizes, 2000 + 10 * k + ns, key_range=sum(sizes) // 3, repeats=True)


def fullest_partition_case(k, a_newest):
    """Partition 1 at max_partition(k) entries.  Run A is 3 * q * 256
    consecutive keys.  Every other run is one entry far below A, 255 keys
    strictly inside the key window of A's share of partition 1 (chosen among
    A's own keys, so the dedup drops one copy of each), and one entry far
    above A: it has two samples, the far ones.  The k - 1 low samples rank
    first, so partition 1 starts at A's sample q - (k - 1) and holds q of A's
    samples, q * 256 entries, and the 255 inside entries of every other run."""
    q = q_of(k)
    rng = np.random.default_rng(3000 + 2 * k + a_newest)
    na = 3 * q * S
    x1, x2 = (q - (k - 1)) * S, (2 * q - (k - 1)) * S  # the keys at partition 1's and 2's start
    ra = 0 if a_newest else k - 1
    runs = [None] * k
    runs[ra] = entries(np.arange(na), ra, rng.random(na) < 0.125)
    others = [r for r in range(k) if r != ra]
    for r in others:
        inside = np.sort(rng.choice(np.arange(x1 + 1, x2), size=S - 1, replace=False))
        keys = np.concatenate([[-1_000_000 - r], inside, [10_000_000 + r]])
        runs[r] = entries(keys, r, rng.random(keys.size) < 0.125)
    return runs


EQUAL_KEYS = (I32_MIN, 0, I32_MAX)


def equal_keys_case(key, first_is_tombstone):
    """k = 3 runs of 600, 300 and 9,000 entries of one key: partition 1 starts
    inside them (in run 2), and its predecessor has the same key."""
    runs = [entries(np.full(n, key), r) for r, n in enumerate((600, 300, 9000))]
    if first_is_tombstone:
        runs[0][0, 1] = TOMB
    return runs


def tombstone_stretch_case():
    """k = 2 runs of 20,000 entries with the same keys; the newer run's
    entries of the middle 14,000 keys are tombstones.  With tombstones dropped
    the partitions inside the stretch keep nothing (both copies go)."""
    n = 20_000
    keys = np.arange(n)
    return [entries(keys, 0, (keys >= 3000) & (keys < 17_000)), entries(keys, 1)]


def disjoint_case(n, descending):
    """k = 4 runs of n entries with disjoint key ranges: run r entirely above
    run r + 1 (descending), or entirely below it."""
    runs = []
    for r in range(4):
        band = 3 - r if descending else r
        runs.append(entries(band * 100_000 + np.arange(n) * 3, r, np.arange(n) % 11 == 0))
    return runs


# --- merge rounds ----------------------------------------------------------
PAIR_SIZES = [(0, 1), (1, 0), (1, 1), (2047, 1), (2048, 0), (1024, 1024), (2049, 2047),
              (4096, 1), (1, 4096), (6000, 6001)]
PAIR_PATTERNS = ("interleaved", "a_first", "b_first", "equal", "ties")


def pair_case(na, nb, pattern):
    """The inputs of one stable merge: a as run 0, b as run 1."""
    if pattern == "interleaved":
        ka, kb = np.arange(na) * 2, np.arange(nb) * 2 + 1
    elif pattern == "a_first":
        ka, kb = np.arange(na), na + np.arange(nb)
    elif pattern == "b_first":
        ka, kb = nb + np.arange(na), np.arange(nb)
    elif pattern == "equal":
        ka, kb = np.full(na, 7), np.full(nb, 7)
    else:  # repeated keys inside and across the inputs
        rng = np.random.default_rng(4000 + na + 3 * nb)
        span = max(2, (na + nb) // 4)
        ka, kb = np.sort(rng.integers(0, span, size=na)), np.sort(rng.integers(0, span, size=nb))
    return entries(ka, 0), entries(kb, 1)


def round_case(np_pairs, empty_at=None):
    """np_pairs pairs of mixed sizes and patterns from the lists above; the
    pair at empty_at (if any) has no entries."""
    pairs = []
    for p in range(np_pairs):
        na, nb = PAIR_SIZES[(3 * p + 2 * np_pairs + 1) % len(PAIR_SIZES)]
        if p == empty_at:
            na = nb = 0
        pairs.append(pair_case(na, nb, PAIR_PATTERNS[(p + np_pairs) % len(PAIR_PATTERNS)]))
    return pairs


# --- dedup -------------------------------------------------------------------
DEDUP_SIZES = (1, 2, 511, 512, 513, 4095, 4096, 4097, 8193)
DEDUP_PATTERNS = ("distinct", "equal", "twice_from_0", "twice_from_1")


def dedup_case(n, pattern):
    """A key-sorted array of n entries; about one in five a tombstone.  The
    twice patterns put an equal pair inside a 16-byte vector (from 0) or
    across two (from 1), and so across the 512-entry rounds and 4,096-entry
    tiles."""
    i = np.arange(n)
    keys = {"distinct": i - n // 2, "equal": np.full(n, -5), "twice_from_0": i // 2,
            "twice_from_1": (i + 1) // 2}[pattern]
    rng = np.random.default_rng(5000 + n)
    return entries(keys, 0, rng.random(n) < 0.2)


# --- more than 8 runs: the pairwise rounds through the API -------------------
MANY_RUNS = (9, 10, 11, 16, 17, 18, 33, 64)


def many_runs_case(nruns):
    """Run j has 1, 2047, 2048, 2049, 4097 or 300 + 7j entries in rotation,
    unique keys from a range of 8,192: most keys are in several runs."""
    sizes = [(1, 2047, 2048, 2049, 4097, 300 + 7 * j)[j % 6] for j in range(nruns)]
    return shared_key_runs(sizes, 6000 + nruns, key_range=8192)


def second_chunk_runs():
    """9 runs of 466,490 entries (4,198,410 in all: past the 1,025 dedup
    tiles at which k_scan_counts takes a second chunk), overlapping keys."""
    n = 466_490
    i = np.arange(n)
    return [entries(i * 2 + (r & 1) + 1000 * r, r, (i * 7 + r) % 5 == 0) for r in range(9)]
