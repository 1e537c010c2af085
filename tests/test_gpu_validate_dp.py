"""Two ranks: a world-2 Trainer.validate over a five-batch split (tests/validate_dp_child.py, the
batches dealt ``[rank::world]``: 3 and 2 of them) equals the single-process pass over all five —
counts exactly, the per-token values within 1e-9 relative (the fp64 sums are formed in another
order).  Children are spawned (never exec'd over a GPU process) and bounded by a timeout."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_children(out):
    port = _port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), MMS2UT_DIST_BACKEND="gloo")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "validate_dp_child.py"), str(out)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace")[-3000:])
    assert all(p.returncode == 0 for p in procs), logs
    return [json.load(open(os.path.join(str(out), f"rank{r}.json"))) for r in range(2)]


def check(ranks, single):
    assert ranks[0] == ranks[1]                      # every rank holds the all-reduced stats
    got = ranks[0]
    assert got["ntokens"] == single["ntokens"] and got["nsentences"] == single["nsentences"] == 11
    assert got["accuracy"] == single["accuracy"]     # exact counts: the same quotient
    for k in ("loss", "nll_loss", "ppl"):
        assert abs(got[k] - single[k]) / abs(single[k]) < 1e-9, (k, got[k], single[k])


def test_world2_validate_equals_world1(tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    import validate_dp_child as child
    check(run_children(tmp_path), child.validate(0, 1))
