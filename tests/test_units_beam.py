"""CPU: the host restatement of the beam decode of speech units (multimodal-s2ut_amd/units.py
beam_decode_host, pairwise_sum) against fixtures written by the reference's own HubertCode.decode
(scripts/gen_units_beam_golden.py), and the limits.  Nothing here needs a GPU or the reference checkout."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, pkg

CASES = sorted(os.path.basename(p)[len("units_beam_"):-len(".npz")]
               for p in glob.glob(os.path.join(GOLDEN, "units_beam_*.npz")))


@pytest.fixture(scope="module")
def U():
    return pkg("units")


def test_fixtures_present():
    assert CASES == ["a", "b", "c", "one", "open"]
    golds = [np.load(os.path.join(GOLDEN, f"units_beam_{c}.npz")) for c in CASES]
    assert all(int(str(g["numpy"]).split(".")[0]) >= 2 for g in golds)          # the float32 evaluation
    assert any(int(g["ties"]) > 0 for g in golds)                               # the stable order is exercised
    assert any(not np.array_equal(g["beam_code"], g["code"]) for g in golds)    # and the beam changes something


@pytest.mark.parametrize("case", CASES)
def test_beam_decode_host_matches_reference(U, case):
    g = np.load(os.path.join(GOLDEN, f"units_beam_{case}.npz"))
    idx, val = g["idx"], g["val"]
    assert idx.shape == val.shape == (len(g["code"]), int(g["top_k"])) and val.dtype == np.float32
    beam = U.beam_decode_host(idx, val, int(g["beamsize"]))
    print(f"{case}: ties in the kept beam {int(g['ties'])}, beam differs from greedy in "
          f"{int((g['beam_code'] != g['code']).sum())} of {len(beam)} frames")
    assert beam == g["beam_code"].tolist()
    assert U.merge(beam) == g["beam_merged_code"].tolist()
    assert [int(c) for c in idx[:, 0]] == g["code"].tolist()


@pytest.mark.parametrize("k", range(1, 33))
def test_pairwise_sum_is_numpy_sum(U, k):
    rows = np.sort(np.random.default_rng(k).random((300, k), dtype=np.float32) * np.float32(7.0), axis=1)
    got = np.array([U.pairwise_sum(r) for r in rows])
    want = np.array([np.sum(r) for r in rows])
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_limits(U):
    idx, val = np.zeros((3, 33), dtype=np.int32), np.ones((3, 33), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="32"):
        U.beam_decode_host(idx, val, 1)
    with pytest.raises(NotImplementedError, match="2048"):
        U.beam_decode_host(idx[:, :10], val[:, :10], 205)
    assert len(U.beam_decode_host(idx[:, :8], val[:, :8], 256)) == 3           # 2048 candidates: the limit itself
    with pytest.raises(ValueError):
        U.beam_decode_host(idx[:, :8], val[:, :8], 0)
    with pytest.raises(NotImplementedError, match="32"):
        U.pairwise_sum(np.ones(33, dtype=np.float32))


def test_zero_or_non_finite_distances_are_refused(U):
    idx = np.zeros((2, 3), dtype=np.int32)
    val = np.ones((2, 3), dtype=np.float32)
    val[1] = 0.0
    with pytest.raises(U.NonFiniteFeatures, match="frame 1"):
        U.beam_decode_host(idx, val, 4)
    val[1] = [1.0, np.inf, 2.0]
    with pytest.raises(U.NonFiniteFeatures, match="frame 1"):
        U.beam_decode_host(idx, val, 4)
