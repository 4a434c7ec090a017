"""GPU: a plain `bench.py` run (no --full) measures the headline and nothing else.  Its line carries the contract's fields,
every record that --full adds is null or absent, and --dump-outputs writes the last timed step's token and logits."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import ROOT  # noqa: E402


def test_plain_run_measures_the_headline_only(tmp_path):
    steps, warmup = 12, 3
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(dump)]
    t0 = time.perf_counter()
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])

    assert line["metric"] == "decode tokens/sec (bs=1)" and line["unit"] == "tokens/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f16" and line["steps"] == steps and line["warmup"] == warmup and line["n_gpus"] == 1
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) < 1e-3

    cfg = line["config"]
    assert cfg["full"] is False and cfg["tok_s_400"] is None and cfg["tok_s_single_step_replay"] is None
    assert line["roofline"] is None and line["cpu_baseline"] is None
    for key in ("roofline_by_shape", "exact_mode_tok_s", "other_configs", "pipeline_70b", "tp_70b"):
        assert key not in line, key

    tok, logits = np.load(dump / "next_token.npy"), np.load(dump / "logits.npy")
    assert tok.dtype == np.float64 and tok.shape == (1, ) and logits.dtype == np.float32 and logits.shape == (128256, )
    assert np.isfinite(logits).all() and 0 <= tok[0] < 128256 and tok[0] == int(tok[0])

    # set-up, the steps and the exit only: far below the minutes the --full records take (a plain run is ~10 s of set-up)
    outside = wall - (steps + warmup) * line["ms_per_step"] / 1e3
    assert outside < 90, "plain run spent %.1f s outside its steps" % outside
