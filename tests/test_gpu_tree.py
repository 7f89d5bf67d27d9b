"""The tree handle on the GPU (bloomhip.LSMTree): after every batch it holds
exactly the tree the reference holds after the same ops put one by one.  The
expected tree comes from the plain Python model of tests/tree_model.py (pinned
against the reference's recorded tests in test_tree_host.py); the filter bits
from the C oracle; one test compares with the reference's own binary."""
import copy
import json
import os
import subprocess

import numpy as np
import pytest

import bloomhip as bh
from tree_model import TOMB, ModelTree, NoMoreSpace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSM_BIN = os.path.join(ROOT, "oracle", "_ref", "lsm_bloomhip")
with open(os.path.join(ROOT, "tests", "golden", "ref_tests.json")) as _f:
    REF_TESTS = json.load(_f)["tests"]


def entries_of(run):
    return np.array(sorted(run.items()), dtype=np.int32).reshape(-1, 2)


def assert_run(got, view, want, m, coracle):
    ents = entries_of(want)
    assert np.array_equal(got, ents)
    assert view.m == m
    keys = np.ascontiguousarray(ents[:, 0])
    if keys.size == 0:  # a run of no keys: no bit set (and nothing to fence)
        assert not view.words().any()
        return
    assert np.array_equal(view.words(), coracle.build(m, keys))
    fences, max_key = view.run_meta()
    hand = bh.BloomFilter(m)
    hand.set_batch_run(keys)
    hf, hm = hand.run_meta()
    assert np.array_equal(fences, hf) and max_key == hm
    assert np.array_equal(fences, keys[::4096]) and max_key == keys[-1]


def assert_parity(tree, model, bpe, coracle, probe_keys=None):
    assert tree.shape() == model.shape()
    got, view = tree.run(-1)
    assert_run(got, view, model.buf, bh.m_bits(model.B, bpe), coracle)
    for l, lv in enumerate(model.levels):
        m = bh.m_bits(model.B * model.fanout ** l, bpe)
        for i, run in enumerate(lv):
            got, view = tree.run(l, i)
            assert_run(got, view, run, m, coracle)
    if probe_keys is not None:
        assert_queries(tree, model, probe_keys)


def assert_queries(tree, model, keys):
    keys = np.asarray(keys, dtype=np.int32)
    vals, found = tree.get(keys)
    want = [model.get(int(k)) for k in keys]
    assert vals.tolist() == [w[0] for w in want]
    assert found.tolist() == [w[1] for w in want]
    lo, hi = int(keys.min()), int(keys.max())
    rng = np.random.default_rng(len(keys) + model.nops)
    a = rng.integers(lo - 2, hi + 2, size=12)
    b = a + rng.integers(-2, hi - lo + 4, size=12)      # some with end <= start
    a[0], b[0] = lo - 5, hi + 5                          # everything
    a[1], b[1] = hi, lo                                  # end < start
    a[2], b[2] = lo, lo                                  # end == start
    dead = [k for k in keys.tolist() if model.get(k)[0] == TOMB and model.get(k)[1] >= 0]
    if dead:                                             # the newest entry is a tombstone
        a[3], b[3] = dead[0], dead[0] + 1
        assert model.range(dead[0], dead[0] + 1) == []
    off, out = tree.range(a.astype(np.int32), b.astype(np.int32))
    for q in range(a.size):
        got = [tuple(r) for r in out[int(off[q]):int(off[q + 1])].tolist()]
        assert got == model.range(int(a[q]), int(b[q])), (q, a[q], b[q])
    assert int(off[-1]) == len(out)


def random_ops(rng, n, domain, deletes=0.2):
    ops = np.empty((n, 2), dtype=np.int32)
    ops[:, 0] = rng.integers(0, domain, size=n) * 3 - domain
    ops[:, 1] = rng.integers(-1000, 1000, size=n)
    ops[rng.random(n) < deletes, 1] = TOMB
    return ops


def model_put(model, ops):
    """The ops through the model; on "No more space" the model is left as it
    was before them and False is returned."""
    saved = copy.deepcopy(model.__dict__)
    try:
        for k, v in ops.tolist():
            model.put(k, v)
        return True
    except NoMoreSpace:
        model.__dict__.update(saved)
        return False


@pytest.mark.parametrize("fanout", [2, 3])
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_parity_with_the_model(B, depth, fanout, coracle):
    """Small trees, 20 % deletes, key domains of B, 2B and 1000 values, 3-5
    seeded batches of 0-120 ops each (fewer where the tree would be full at
    once): shape, every run's entries, filter words, fences and max key, the
    memtable, GET of every key of the domain and a set of ranges, after every
    batch.  A batch the reference would die on leaves the tree unchanged."""
    bpe = 10.0  # m = (long)(B * bpe) >= 1 at B = 1
    capacity = sum(fanout ** (l + 1) for l in range(depth))
    for domain in (B, 2 * B, 1000):
        rng = np.random.default_rng(B * 1000 + depth * 100 + fanout * 10 + domain)
        tree = bh.LSMTree(B, depth, fanout, bpe)
        model = ModelTree(B, depth, fanout)
        probe = np.arange(0, min(domain, 200)) * 3 - domain
        ok = 0
        for batch in range(int(rng.integers(3, 6))):
            n = int(rng.integers(0, min(120, B * capacity) + 1))
            ops = random_ops(rng, n, domain)
            before = len(model.cuts)
            if model_put(model, ops):
                assert tree.put_batch(ops) == len(model.cuts) - before
                ok += 1
            else:
                with pytest.raises(bh.BloomHipError) as ei:
                    tree.put_batch(ops)
                assert ei.value.status == bh.ERANGE
            assert_parity(tree, model, bpe, coracle, probe)
        assert ok >= 1
        tree.close()


def test_old_runs_only_merge_and_an_empty_last_level_run(coracle):
    """B = 2, depth 3, fanout 2.  Thirteen deletes make six flushes: two runs
    in level 0, two merged runs in level 1 holding tombstones only (kept in the
    middle level).  The next batch's first flush merges level 1 down before
    anything new lands there: a run made of old runs only, into the last level,
    where every tombstone is dropped; the run ends empty and keeps its slot."""
    bpe = 10.0
    tree, model = bh.LSMTree(2, 3, 2, bpe), ModelTree(2, 3, 2)
    ops = np.array([[k, TOMB] for k in range(13)], dtype=np.int32)
    assert model_put(model, ops) and tree.put_batch(ops) == 6
    assert tree.shape() == ([2, 2, 0], 1)
    assert_parity(tree, model, bpe, coracle, np.arange(-1, 15))
    assert tree.run(1, 1)[0].tolist() == [[k, TOMB] for k in range(4)]
    ops = np.array([[100, 1], [101, 2], [0, 5]], dtype=np.int32)
    assert model_put(model, ops) and tree.put_batch(ops) == 1
    assert tree.shape() == ([1, 1, 1], 2) == model.shape()
    ents, view = tree.run(2, 0)
    assert ents.shape == (0, 2) and not view.words().any()
    assert_parity(tree, model, bpe, coracle, np.arange(-1, 15))
    # buffer 0, level 0's run 1, level 1's run 2; keys 0..7 left the tree with their tombstones
    vals, found = tree.get(np.array([100, 12, 9, 5, 0, 3], dtype=np.int32))
    assert found.tolist() == [1, 1, 2, -1, 0, -1] and vals.tolist() == [1, TOMB, TOMB, TOMB, 5, TOMB]
    tree.close()


def test_no_more_space_leaves_the_tree_unchanged(coracle):
    bpe = 10.0
    tree, model = bh.LSMTree(3, 2, 2, bpe), ModelTree(3, 2, 2)
    rng = np.random.default_rng(3)
    ops = random_ops(rng, 16, 1000, deletes=0.0)
    ops[:, 0] = np.arange(16) * 5              # distinct: five flushes, one op in the buffer
    assert model_put(model, ops) and tree.put_batch(ops) == 5
    assert tree.shape() == ([1, 2], 1)
    # six flushes fit (2 + 2 * 2); the batch below makes two more
    more = ops.copy()
    more[:, 0] += 1000
    assert not model_put(model, more[:7])
    with pytest.raises(bh.BloomHipError) as ei:
        tree.put_batch(more[:7])
    assert ei.value.status == bh.ERANGE
    assert_parity(tree, model, bpe, coracle, ops[:, 0])
    # one more flush still fits, and the tree goes on from where it was
    assert model_put(model, more[:4]) and tree.put_batch(more[:4]) == 1
    assert_parity(tree, model, bpe, coracle, np.concatenate([ops[:, 0], more[:4, 0]]))
    tree.close()


def test_parity_b512(coracle):
    """The reference's -b 1 buffer: B = 512, depth 3, fanout 2, three batches."""
    tree, model = bh.LSMTree(512, 3, 2, 0.5), ModelTree(512, 3, 2)
    rng = np.random.default_rng(512)
    for n in (700, 2500, 1200):
        ops = random_ops(rng, n, 4000)
        before = len(model.cuts)
        assert model_put(model, ops)
        assert tree.put_batch(ops) == len(model.cuts) - before
        assert_parity(tree, model, 0.5, coracle, np.arange(0, 4000, 7) * 3 - 4000)
    assert len(model.cuts) >= 6
    tree.close()


def test_parity_large_buffer(coracle):
    """B = 2 * FLUSH_BLOCK_CAP: every segment goes down the tiled sort; three
    flushes, the third merging the first two into level 1 (several fences)."""
    B = 2 * bh.FLUSH_BLOCK_CAP
    tree, model = bh.LSMTree(B, 2, 2, 0.5), ModelTree(B, 2, 2)
    rng = np.random.default_rng(99)
    ops = random_ops(rng, 3 * B + B // 2, 1 << 20, deletes=0.1)
    assert model_put(model, ops)
    assert len(model.cuts) == 3
    assert tree.put_batch(ops) == 3
    assert tree.shape()[0] == [1, 1]
    assert_parity(tree, model, 0.5, coracle, ops[::97, 0])
    tree.close()


def test_device_ops_and_load(tmp_path, coracle):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(17)
    ops = random_ops(rng, 200, 200)
    tree, model = bh.LSMTree(8, 3, 3, 10.0), ModelTree(8, 3, 3)
    assert model_put(model, ops[:100])
    tree.put_batch(torch.from_numpy(ops[:100]).cuda())
    path = tmp_path / "data.bin"
    ops[100:].tofile(path)
    assert model_put(model, ops[100:])
    tree.load(str(path))
    assert_parity(tree, model, 10.0, coracle, np.arange(200) * 3 - 200)
    keys = torch.from_numpy(np.ascontiguousarray(ops[:64, 0])).cuda()
    vals = torch.empty(64, dtype=torch.int32, device="cuda")
    found = torch.empty(64, dtype=torch.int32, device="cuda")
    tree.get(keys, vals=vals, found_run=found)
    want = [model.get(int(k)) for k in ops[:64, 0]]
    assert vals.cpu().tolist() == [w[0] for w in want]
    assert found.cpu().tolist() == [w[1] for w in want]
    tree.close()


def answer_lines(tree, ops):
    """The stdout lines of the reference for `ops` (fixture form), puts going in
    as one batch up to each g or r op (src/lsm_tree.cpp:173-290 for the format)."""
    lines, pending = [], []

    def flush_pending():
        if pending:
            tree.put_batch(np.array(pending, dtype=np.int32).reshape(-1, 2))
            pending.clear()

    for op in ops:
        if op[0] == "p":
            pending.append((op[1], op[2]))
        elif op[0] == "d":
            pending.append((op[1], TOMB))
        elif op[0] == "g":
            flush_pending()
            vals, _ = tree.get(np.array([op[1]], dtype=np.int32))
            lines.append("" if vals[0] == TOMB else str(vals[0]))
        elif op[0] == "r":
            flush_pending()
            _, out = tree.range(np.array([op[1]], np.int32), np.array([op[2]], np.int32))
            lines.append(" ".join(f"{k}:{v}" for k, v in out.tolist()))
    flush_pending()
    return lines


@pytest.mark.parametrize("name", ["test-5", "test-6"])
def test_recorded_reference_tests(name):
    t = REF_TESTS[name]
    assert t["params"] == ["-b", "1"]
    tree = bh.LSMTree(512)
    want = t["expected_stdout"].split("\n")
    assert answer_lines(tree, t["ops"]) == [w.rstrip(" ") for w in want[:-1]]
    tree.close()


needs_lsm = pytest.mark.skipif(not os.access(LSM_BIN, os.X_OK),
                               reason="oracle/_ref/lsm_bloomhip not built (no reference tree)")


@needs_lsm
def test_against_the_reference_binary(tmp_path):
    """The reference's own LSM (-b 1 -d 3 -f 2) on about 40,000 ops in three
    batches, 500 gets and 20 ranges after each.  Keys come from exactly 512
    values and 10 % of the ops are deletes, so no run, merged or not, passes 512
    entries: up to there the reference's 4096-byte page window reads the right
    entries.  Filling the buffer then takes about 512 ln 512 + 0.58 * 512 =
    3,500 ops, so the stream makes about 11 of the 14 flushes the tree takes.
    The same window also reads the slots past the end of a run shorter than 512
    entries (a last-level run that lost its tombstones), which hold key 0 and
    value 0: the keys and every query are positive, so no such slot is in range."""
    rng = np.random.default_rng(4242)
    domain = np.arange(512) * 13 + 1000
    ops, model = [], ModelTree(512, 3, 2)
    for batch in range(3):
        n = 13_300 + batch
        keys = domain[rng.integers(0, 512, size=n)]
        vals = rng.integers(-100_000, 100_000, size=n)
        dele = rng.random(n) < 0.1
        for k, v, d in zip(keys.tolist(), vals.tolist(), dele.tolist()):
            ops.append(("d", k) if d else ("p", k, v))
            model.put(k, TOMB if d else v)
        ops += [("g", int(k)) for k in rng.integers(990, 7670, size=500)]
        a = rng.integers(990, 7670, size=20)
        b = a + rng.integers(-50, 1500, size=20)
        ops += [("r", int(x), int(y)) for x, y in zip(a, b)]
    assert 8 <= len(model.cuts) <= 14, len(model.cuts)
    assert max(len(r) for r in model.runs()) <= 512
    tree = bh.LSMTree(512, 3, 2)
    got = answer_lines(tree, ops)
    assert tree.shape() == model.shape()
    tree.close()
    text = "\n".join(" ".join(str(x) for x in op) for op in ops) + "\n"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(
        p for p in (bh.LIB_DIR, env.get("LD_LIBRARY_PATH")) if p)
    r = subprocess.run([LSM_BIN, "-b", "1", "-d", "3", "-f", "2"], input=text, capture_output=True,
                       text=True, cwd=tmp_path, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    want = r.stdout.split("\n")
    assert want[-1] == "" and len(want) - 1 == 3 * 520
    want = [w.rstrip(" ") for w in want[:-1]]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (bad[:5], got[bad[0]][:200], want[bad[0]][:200])
