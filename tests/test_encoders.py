"""CPU: the weight images the three encoders pack at load (asr.py, units.py, vision.py through encoders.py)
against tests/golden/encoder_images.json -- every tensor's name, dtype, shape and the sha256 of its bytes,
exactly.  scripts/gen_encoder_image_golden.py builds the models here as it did for the golden."""
import importlib.util
import json
import os

from conftest import GOLDEN, ROOT


def test_packed_weight_images_match_the_golden():
    spec = importlib.util.spec_from_file_location("gen_encoder_image_golden",
                                                  os.path.join(ROOT, "scripts", "gen_encoder_image_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "encoder_images.json")) as f:
        want = json.load(f)
    got = gen.images()
    assert sorted(got) == sorted(want) == ["hubert", "hubert_bias", "hubert_no_fp_ln", "vit", "wav2vec2"]
    for model in want:
        assert sorted(got[model]) == sorted(want[model]), model
        for name, w in want[model].items():
            assert got[model][name] == w, (model, name)
    # what the variants are about: the conv biases and the feature projection's LayerNorm come and go
    assert want["hubert"]["conv3.b"] is None and want["hubert_bias"]["conv3.b"] is not None
    assert "fp_g" in want["hubert"] and "fp_g" not in want["hubert_no_fp_ln"]
