"""bench.py's launch contract (CPU only, no GPU touched).

`python bench.py --gpus N` must either measure N GPUs or fail: it starts N
ranks itself when no launcher set WORLD_SIZE (one process per
GPU), refuses a WORLD_SIZE that differs from --gpus, and propagates a rank's
failure as its own non-zero exit status.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra, timeout=120):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True,
                          text=True, timeout=timeout)


def test_world_size_mismatch_exits_nonzero():
    r = _run(["--gpus", "2"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2, r.stderr
    assert "WORLD_SIZE=1 but --gpus 2" in r.stderr
    r = _run(["--gpus", "1"], {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2, r.stderr


def test_bad_gpu_count_exits_nonzero():
    r = _run(["--gpus", "0"], {})
    assert r.returncode == 2


def test_self_launch_starts_ranks_and_propagates_failure():
    # No GPU here: the two ranks it starts fail at device selection, and the
    # parent must report that as a non-zero exit, never as a 1-GPU line.
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-extras",
              "--no-cpu-baseline", "--prewarm-s", "0"], {"BLOOMHIP_DIST_BACKEND": "gloo"})
    assert r.returncode != 0
    assert "exited with" in r.stderr
    assert '"n_gpus": 1' not in r.stdout


def test_launch_ranks_sets_rank_environment(tmp_path, monkeypatch):
    # launch_ranks re-runs bench.py; point it at a stand-in script that
    # reports the rank environment it was given.
    sys.path.insert(0, ROOT)
    import bench
    probe = tmp_path / "probe.py"
    out = tmp_path / "ranks"
    out.mkdir()
    probe.write_text(
        "import os, sys\n"
        f"open(os.path.join({str(out)!r}, os.environ['RANK']), 'w').write(\n"
        "    ' '.join(os.environ[k] for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', "
        "'MASTER_ADDR')) + ' ' + ' '.join(sys.argv[1:]))\n")
    monkeypatch.setattr(bench, "__file__", str(probe))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "3", "--steps", "7"])
    assert bench.launch_ranks(3) == 0
    got = sorted(p.read_text() for p in out.iterdir())
    assert got == [f"{r} {r} 3 127.0.0.1 --gpus 3 --steps 7" for r in range(3)]


def test_bad_step_count_exits_nonzero():
    r = _run(["--gpus", "1", "--steps", "0"], {})
    assert r.returncode == 2
    assert "--steps must be >= 1" in r.stderr


def _words_from_u16(a):
    import numpy as np
    assert a.dtype == np.float32
    return a.astype(np.uint16).view(np.uint64)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    # The dump is exact (every uint64 word recoverable from its float32
    # 16-bit parts), and a bitmap over the budget is sampled at indices that
    # depend on nothing but its size.
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    words = np.random.default_rng(5).integers(0, 1 << 64, size=5000, dtype=np.uint64)
    bench.dump_outputs(str(tmp_path / "whole"), words)
    assert sorted(os.listdir(tmp_path / "whole")) == ["bitmap_u16.npy"]
    assert (_words_from_u16(np.load(tmp_path / "whole" / "bitmap_u16.npy")) == words).all()

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 16 * words.size - 1)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_WORDS", 300)
    got = []
    for name in ("a", "b"):
        d = tmp_path / name
        bench.dump_outputs(str(d), words)
        assert sorted(os.listdir(d)) == ["bitmap_sample_index.npy", "bitmap_sample_u16.npy"]
        idx = np.load(d / "bitmap_sample_index.npy")
        assert idx.dtype == np.float64 and idx.size == 300 and (np.diff(idx) > 0).all()
        assert (_words_from_u16(np.load(d / "bitmap_sample_u16.npy"))
                == words[idx.astype(np.int64)]).all()
        got.append(idx)
    assert (got[0] == got[1]).all()


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_pinned_bitmap(tmp_path, golden):
    # A plain run: the headline fields, none of the --full legs, and the
    # bitmap of the last timed step equal to the oracle's C2 pin.
    import hashlib
    import json

    import numpy as np
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm-s", "0",
              "--dump-outputs", str(tmp_path / "out")], {})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "Gkeys/s" and d["higher_is_better"] is True and d["value"] > 0
    assert d["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region
    n = d["config"]["keys_per_run"]
    assert abs(d["value"] - n / (d["ms_per_step"] * 1e-3) / 1e9) <= 1e-3 * d["value"]
    assert d["cpu_baseline"] is None and d["kernels"] == {}
    for leg in ("c5_eight_runs", "c1_check", "c4_build", "probe_c3", "f10", "route_c3",
                "compact_fanin4", "e2e_build", "scalar_is_set", "cpu_baseline_detail"):
        assert leg not in d
    words = _words_from_u16(np.load(tmp_path / "out" / "bitmap_u16.npy"))
    assert hashlib.sha256(words.tobytes()).hexdigest() == golden["oracle"]["c2"]["sha256"]
