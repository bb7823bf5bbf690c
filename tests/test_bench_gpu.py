"""bench.py's contract for a plain run: --steps sets the timed steps, the line carries ms_per_step and none of the --full
sections, and --dump-outputs writes the logits of the timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_logits(tmp_path):
    import bench
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "tokens/s" and line["higher_is_better"] is True and "fp8_e4m3" in line["dtype"]
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - bench.MAX_NUM_SEQS * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
    for key in ("ttft_p50_ms", "engine_decode_tokens_per_s", "roofline", "cpu_baseline", "speculation"):
        assert key not in line, key
    assert os.listdir(out) == ["logits.npy"]
    logits = np.load(out / "logits.npy")
    assert logits.dtype == np.float32 and logits.shape == (bench.MAX_NUM_SEQS, bench.MODELS["llama31_8b"]["vocab_size"])
    assert np.isfinite(logits).all() and logits.std() > 0
