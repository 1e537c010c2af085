"""CPU: tests/asr_ref.py's wav2vec2 restatement against logits of the ``transformers`` library's own
Wav2Vec2ForCTC (tests/golden/w2v2_hf_small_logits.npz, written by scripts/gen_hf_golden.py with the same
seeded weights).  Nothing here imports ``transformers``."""
import os

import numpy as np
import torch

import asr_ref as AR
import hubert_ref as HR
from conftest import GOLDEN
from test_units import HF_TOL, check_checksums


def test_asr_restatement_matches_hf_golden():
    gold = np.load(os.path.join(GOLDEN, "w2v2_hf_small_logits.npz"))
    sd = AR.make_state_dict(AR.SMALL, 0, style="param")
    check_checksums(gold, sd, "w2v2_hf_small_logits")
    for n, ws in HR.WAVES:
        with torch.no_grad():
            got = AR.forward(sd, AR.SMALL, AR.to_float(AR.make_wave(n, ws)))
        ref = torch.from_numpy(gold[f"logits_{n}"])
        assert got.shape == ref.shape
        err = float((got - ref).abs().max())
        print(f"wav2vec2 n{n}: max-abs vs HF {err:.2e} (logit scale {float(ref.abs().max()):.2f})")
        assert err <= HF_TOL, (n, err)
