"""bench.py as a program: a plain run prints the headline line and nothing else, `--steps` sets the timed steps, `--dump-outputs`
writes the last step's layer roots, `--full` adds the golden checks.  The GPU runs use the 2^10-row trace, whose roots the CPU
oracle recorded in tests/golden/step_roots_k10.json."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD10 = os.path.join(ROOT, "tests", "golden", "step_roots_k10.json")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args, timeout=300):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    return out.returncode, out.stdout, out.stderr


def _line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_roots_words_are_the_exact_limbs():
    """The dump format: each root's four u64 limbs as eight 32-bit words in float64, least significant first — no bit lost."""
    sys.path.insert(0, ROOT)
    import bench
    hexes = json.load(open(GOLD10))["roots"]
    roots = [np.array([(int(h, 16) >> (64 * i)) & (2**64 - 1) for i in range(4)], np.uint64) for h in hexes]
    assert bench.roots_hex(roots) == hexes
    w = bench.roots_words(roots)
    assert w.dtype == np.float64 and w.shape == (len(hexes), 8)
    back = [sum(int(x) << (32 * j) for j, x in enumerate(row)) for row in w]
    assert back == [int(h, 16) for h in hexes]


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"], ["--csv", "x.csv"]])
def test_bad_arguments_are_refused_before_any_device_work(args):
    rc, _, err = _bench(*args, timeout=60)
    assert rc == 2 and "error" in err


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    rc, out, err = _bench("--steps", "3", "--warmup", "1", "--log-trace", "10", "--dump-outputs", str(tmp_path / "dump"))
    assert rc == 0, err[-2000:]
    line = _line(out)
    for key in HEADLINE:
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx((1 << 10) / (line["ms_per_step"] * 1e-3))
    assert "roots_match_golden" not in line and "roofline" not in line and "cpu_baseline" not in line
    gold = json.load(open(GOLD10))["roots"]
    assert line["roots"] == gold
    sys.path.insert(0, ROOT)
    import bench
    got = np.load(tmp_path / "dump" / "roots.npy")
    assert got.dtype == np.float64
    want = bench.roots_words([np.array([(int(h, 16) >> (64 * i)) & (2**64 - 1) for i in range(4)], np.uint64) for h in gold])
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_full_steps_only_checks_the_roots_against_the_golden():
    rc, out, err = _bench("--full", "--steps-only", "--steps", "1", "--warmup", "0", "--log-trace", "10")
    assert rc == 0, err[-2000:]
    line = _line(out)
    assert line["roots_match_golden"] is True and line["roots_match_one_gpu_run"] is None
