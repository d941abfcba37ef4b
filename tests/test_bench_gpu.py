"""bench.py's two kinds of run on the GPU: a plain run times the headline only, --full adds the checks (and the other legs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--n", "2000"]
                       + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_line_carries_the_headline_only():
    line = _line()
    assert line["full"] is False and line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "assignments/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["n_gpus"] == 1
    assert line["parity"] is None and line["cpu_baseline"] is None and line["roofline"]["floor_bytes_per_solve"] == 4.0 * 2000 ** 2
    assert not {"c2", "c2_batch", "c2_cytolike", "c3", "c4_chunks", "c5_chunks", "c4_strong", "c4_sharded"} & set(line)


@pytest.mark.gpu
def test_full_bench_line_checks_the_headline():
    # --full without the other legs: the n = 3 000 gate against both CPU oracles and the headline's full-size properties
    line = _line("--full", "--no-extras", "--no-cpu-baseline")
    p = line["parity"]
    assert line["full"] is True and p["bit_exact_vs_cpu_oracle_n3000"] is True
    assert p["full_size_permutation"] and p["full_size_total_1e-5"] and p["full_size_dual_feasible"]
