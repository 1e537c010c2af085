"""The plain bench run (`bench.py --gpus 1 --steps K --warmup W`) and --dump-outputs: one short run,
started once.  The line carries the headline figure and nothing that takes a pass of its own (those
sit behind --full); the dump is float32 .npy files of the last timed step's outputs, at most 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path_factory.mktemp("bench_dump")
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = p.stdout.decode(errors="replace")
    assert p.returncode == 0, text[-3000:]
    lines = [ln for ln in text.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, text[-3000:]
    return json.loads(lines[0]), out


def test_plain_line(run):
    r, _ = run
    assert r["unit"] == "audio-frames/s" and r["higher_is_better"] is True and r["dtype"] == "fp16"
    assert r["steps"] == 2 and r["warmup"] == 1 and r["n_gpus"] == 1
    assert r["value"] > 0 and r["ms_per_step"] > 0
    # frames/s and ms_per_step describe the same window
    assert r["value"] == pytest.approx(r["config"]["global_batch_frames_per_step"] / (r["ms_per_step"] / 1e3), rel=1e-9)
    assert r["optimizer"]["step"] >= 1 and not r["optimizer"]["fatal"]
    for k in ("roofline", "cpu_baseline"):          # --full only
        assert k not in r
    assert "master_checksum" not in r["optimizer"]


def test_dump_outputs(run):
    _, out = run
    files = sorted(os.listdir(out))
    assert files == sorted(n + ".npy" for n in ("log", "src", "ost", "params_sample", "master_sample",
                                                "exp_avg_sample", "exp_avg_sq_sample"))
    arrays = {f[:-4]: np.load(os.path.join(out, f)) for f in files}
    assert all(a.dtype == np.float32 for a in arrays.values())
    # ost is left out: its grad-norm slot is inf on a step the fp16 loss scaler skips, which a window
    # this short may still contain
    bad = [k for k, a in arrays.items() if k != "ost" and not np.isfinite(a).all()]
    assert not bad, bad
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    log = arrays["log"]                             # loss, nll, ntokens, nsentences, ntokens / world
    assert log.shape == (5,) and log[0] > 0 and log[2] > 0 and log[3] == arrays["src"].shape[0]
    n = arrays["params_sample"].size                # the same sampled indices of every flat buffer
    assert all(arrays[k].shape == (n,) for k in ("master_sample", "exp_avg_sample", "exp_avg_sq_sample"))
    # the fp16 parameters are the rounded fp32 master; the second moment is non-negative and not all zero
    assert np.array_equal(arrays["params_sample"], arrays["master_sample"].astype(np.float16).astype(np.float32))
    assert (arrays["exp_avg_sq_sample"] >= 0).all() and arrays["exp_avg_sq_sample"].max() > 0
