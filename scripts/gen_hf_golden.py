"""Golden fixtures from the ``transformers`` library's own HubertModel and Wav2Vec2ForCTC, on CPU.

Run by hand where ``transformers`` is installed; never by a test and never on a GPU machine (the tests
read the committed .npz files and import nothing of the library).  The models are built from the configs
of tests/hubert_ref.py / tests/asr_ref.py and loaded with those files' seeded state dicts; the weights are
not stored, only a float64 checksum (sum, sum of squares) of every tensor, so that a drift of the seeded
generator shows as a checksum mismatch and not as a parity failure.

  tests/golden/hubert_hf_small_<variant>.npz   variant: plain (do_normalize false), norm (true), bias
      (conv_bias true).  Per wave (8000, 1), (12345, 2), (48000, 3) of asr_ref.make_wave:
      hk_<n> = hidden_states[km_layer] (fp32 [T, d]); h0_<n> = every 4th frame of hidden_states[0];
      layer0_8000 = every 16th frame of the first conv layer's output [T0, C] (the files stay small; every
      frame of hk depends on every frame before it); sum_<key> = the checksums; km_layer, normalize.
  tests/golden/w2v2_hf_small_logits.npz        logits_<n> of Wav2Vec2ForCTC for asr_ref.SMALL with
      asr_ref.make_state_dict(SMALL, 0, style="param"); sum_<key>.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_hf_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")
H0_EVERY, LAYER0_EVERY = 4, 16


def _hf_input(x, normalize):
    # Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm, as the processor applies it to one utterance
    if normalize:
        x = (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7)
    return x[None]


def main():
    try:
        import transformers
        from transformers import HubertConfig, HubertModel, Wav2Vec2Config, Wav2Vec2ForCTC
    except ImportError:
        print("transformers is not installed: nothing written", file=sys.stderr)
        return 1
    import asr_ref as AR
    import hubert_ref as HR

    torch.manual_seed(0)
    os.makedirs(OUT, exist_ok=True)
    km = HR.KM_LAYER["small"]
    for variant, over, normalize in (("plain", {}, False), ("norm", {}, True), ("bias", {"conv_bias": True}, False)):
        cfg = dict(HR.SMALL, **over)
        sd = HR.make_state_dict(cfg, 0)
        model = HubertModel(HubertConfig(**cfg, attn_implementation="eager"))
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not missing and not unexpected, (missing, unexpected)
        model.eval()
        out = {"km_layer": np.int64(km), "normalize": np.int64(normalize)}
        out.update({"sum_" + k: v for k, v in HR.checksums(sd).items()})
        for n, ws in HR.WAVES:
            x = _hf_input(AR.to_float(AR.make_wave(n, ws)), normalize)
            with torch.no_grad():
                hs = model(x, output_hidden_states=True).hidden_states
                out[f"h0_{n}"], out[f"hk_{n}"] = hs[0][0][::H0_EVERY].numpy(), hs[km][0].numpy()
                if n == 8000:
                    y0 = model.feature_extractor.conv_layers[0](x[:, None])[0].t()
                    out[f"layer0_{n}"] = y0[::LAYER0_EVERY].contiguous().numpy()
        path = os.path.join(OUT, f"hubert_hf_small_{variant}.npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path)} bytes (transformers {transformers.__version__})")

    sd = AR.make_state_dict(AR.SMALL, 0, style="param")
    model = Wav2Vec2ForCTC(Wav2Vec2Config(**AR.SMALL, attn_implementation="eager"))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    model.eval()
    out = {"sum_" + k: v for k, v in HR.checksums(sd).items()}
    for n, ws in HR.WAVES:
        with torch.no_grad():
            out[f"logits_{n}"] = model(_hf_input(AR.to_float(AR.make_wave(n, ws)), True)).logits[0].numpy()
    path = os.path.join(OUT, "w2v2_hf_small_logits.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
