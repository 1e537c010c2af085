"""CPU: the ViT feature extractor's host side (multimodal-s2ut_amd/vision.py) and the restatement the GPU
tests compare with (tests/vit_ref.py).

The resample restatement is pinned bit for bit to Pillow's own results (tests/golden/vit_pillow_s48.npz) and,
where PIL imports, to the live library; the product's coefficient tables to the restatement's.  The ViT
restatement, run in float64, is compared with the ``transformers`` library's fp32 ViTModel output
(tests/golden/vit_hf_small.npz, scripts/gen_vit_golden.py): allowance TOL_FACTOR x max|HF fp32 - HF double|
from the same file (2.24e-6 when the file was written; the restatement was 1.6e-7 from HF's double run).
Nothing here imports ``transformers``."""
import os

import numpy as np
import pytest
import torch

import asr_ref as AR
import vit_ref as VR
from conftest import GOLDEN, pkg


@pytest.fixture(scope="module")
def V():
    return pkg("vision")


# ------------------------------------------------------------------------------------------ resample

def test_resample_restatement_matches_pillow_golden():
    gold = np.load(os.path.join(GOLDEN, "vit_pillow_s48.npz"))
    assert sorted(k for k in gold.files if k.startswith("u8_")) == sorted(f"u8_{w}x{h}" for w, h in VR.SIZES_48)
    for w, h in VR.SIZES_48:
        got = VR.transform_u8(VR.make_image(w, h, 0), 48)
        assert got.dtype == np.uint8 and got.shape == (48, 48, 3)
        assert np.array_equal(got, gold[f"u8_{w}x{h}"]), (w, h)


@pytest.mark.parametrize("w,h,S", [(w, h, 48) for w, h in VR.SIZES_48] +
                         [(500, 375, 384), (375, 500, 384), (1024, 683, 384), (400, 384, 384), (384, 384, 384), (100, 60, 32)])
def test_resample_restatement_matches_live_pillow(w, h, S):
    pytest.importorskip("PIL")
    im = VR.make_image(w, h, 1)
    assert np.array_equal(VR.transform_u8(im, S), VR.pillow_transform_u8(im, S))


@pytest.mark.parametrize("w,h,S", [(w, h, 48) for w, h in VR.SIZES_48] + [(500, 375, 384), (1024, 683, 384), (100, 60, 32)])
def test_product_tables_match_restatement(V, w, h, S):
    """vision.resample_rows (vectorised, the cropped window only) against vit_ref.coefficients (Pillow's loop)."""
    w2, h2 = V.resize_size(w, h, S)
    assert (w2, h2) == VR.resize_size(w, h, S) and min(w2, h2) == S
    for insize, outsize in ((w, w2), (h, h2)):
        lo = V.crop_origin(outsize, S)
        assert lo == VR.crop_origin(outsize, S) and 0 <= lo <= outsize - S
        first, taps, coef = V.resample_rows(insize, outsize, lo, S)
        assert first.dtype == taps.dtype == coef.dtype == np.int32
        if insize == outsize:      # Pillow skips the pass: the identity table
            assert first.tolist() == list(range(lo, lo + S)) and set(taps.tolist()) == {1}
            assert set(coef.reshape(-1).tolist()) == {1 << 22}
            continue
        for i, (xmin, k) in enumerate(VR.coefficients(insize, outsize)[lo:lo + S]):
            assert (first[i], taps[i]) == (xmin, len(k)) and coef[i, :len(k)].tolist() == k
            assert not coef[i, len(k):].any() and xmin + len(k) <= insize


def test_resize_and_crop_rules(V):
    assert V.resize_size(500, 375, 384) == (512, 384) and V.resize_size(375, 500, 384) == (384, 512)
    assert V.resize_size(400, 384, 384) == (400, 384) and V.resize_size(384, 999, 384) == (384, 999)
    assert V.resize_size(31, 300, 48) == (48, 464)
    # round half to even: (w' - S) / 2 = 0.5, 1.5, 2.5 -> 0, 2, 2
    assert [V.crop_origin(s, 48) for s in (49, 51, 53, 48, 50)] == [0, 2, 2, 0, 1]


def test_norm_table(V):
    t = V.norm_table((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    u = torch.arange(256, dtype=torch.float32) / 255
    assert t.dtype == torch.float16 and t.shape == (3, 256)
    assert torch.equal(t[1], ((u - 0.5) / 0.5).half())
    t = V.norm_table((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    assert torch.equal(t[2], ((u - 0.406) / 0.225).half())
    with pytest.raises(ValueError):
        V.norm_table((0.5, 0.5), (0.5, 0.5, 0.5))


# ------------------------------------------------------------------------------------------ HF golden

def test_vit_restatement_matches_hf_golden():
    gold = np.load(os.path.join(GOLDEN, "vit_hf_small.npz"))
    sd = VR.make_state_dict(VR.SMALL, 0)
    want = {k[4:]: gold[k] for k in gold.files if k.startswith("sum_")}
    assert sorted(want) == sorted(sd)
    have = VR.checksums(sd)
    drift = [k for k in want if not np.allclose(have[k], want[k], rtol=1e-9, atol=1e-12)]
    assert not drift, (f"the seeded weight generator drifted from the one the golden was written with ({drift[:3]}...); "
                       "regenerate with scripts/gen_vit_golden.py. This is not a parity failure.")
    x = VR.pixels([VR.make_image(w, h, s) for w, h, s in VR.GOLDEN_IMAGES], VR.SMALL["image_size"])
    assert np.allclose([float(x.double().sum()), float(x.double().pow(2).sum())], gold["pix_sum"], rtol=1e-9)
    with torch.no_grad():
        got = VR.forward({k: v.double() for k, v in sd.items()}, VR.SMALL, x.double())
    ref32, ref64, noise = torch.from_numpy(gold["out32"]).double(), torch.from_numpy(gold["out64"]), float(gold["noise"])
    assert got.shape == ref32.shape == (2, 10, 128)
    assert noise == float((ref32 - ref64).abs().max()) and noise > 0
    err = float((got - ref32).abs().max())
    print(f"ViT restatement (fp64) vs HF fp32: {err:.2e}; vs HF double {float((got - ref64).abs().max()):.2e}; "
          f"HF fp32 vs double {noise:.2e}; output scale {float(ref64.abs().max()):.2f}")
    assert err <= VR.TOL_FACTOR * noise, (err, noise)


# ------------------------------------------------------------------------------------------ config and loading

def test_model_table(V):
    want = {"vit_tiny_patch16_384": (192, 3, 12), "vit_small_patch16_384": (384, 6, 12),
            "vit_base_patch16_384": (768, 12, 12), "vit_large_patch16_384": (1024, 16, 24)}
    for name, (d, H, L) in want.items():
        c = V.model_config(name)
        assert (c["d"], c["heads"], c["layers"], c["mlp"], c["image_size"], c["patch"]) == (d, H, L, 4 * d, 384, 16)
        assert d // H == 64
    with pytest.raises(ValueError):
        V.model_config("vit_base_patch32_384")


@pytest.mark.parametrize("wrap", [None, "state_dict", "model"])
def test_load_checkpoint_wrapped(V, tmp_path, wrap):
    sd = VR.make_state_dict(VR.SMALL, 0)
    path = str(tmp_path / "ckpt.pth")
    torch.save(sd if wrap is None else {wrap: sd, "epoch": 3}, path)
    got = V.load_checkpoint(path)
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


def test_load_checkpoint_safetensors_and_refusals(V, tmp_path):
    sd = VR.make_state_dict(VR.SMALL, 0)
    path = str(tmp_path / "model.safetensors")
    AR.write_safetensors(path, sd)
    got = V.load_checkpoint(path)
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(NotImplementedError):
        V.load_checkpoint(str(tmp_path / "augreg.npz"))
    torch.save([1, 2, 3], str(tmp_path / "list.pth"))
    with pytest.raises(ValueError):
        V.load_checkpoint(str(tmp_path / "list.pth"))


def test_constructor_checks_shapes_and_keys(V):
    cfg = VR.SMALL
    sd = VR.make_state_dict(cfg, 0)
    bad = dict(sd)
    bad["blocks.1.mlp.fc1.weight"] = torch.zeros(cfg["mlp"], cfg["d"] + 8)
    with pytest.raises(ValueError, match="blocks.1.mlp.fc1.weight"):
        V.ViTFeatures(bad, cfg, device="cpu")
    bad = dict(sd)
    bad["pos_embed"] = torch.zeros(1, 5, cfg["d"])          # another image size: no interpolation
    with pytest.raises(ValueError, match="pos_embed"):
        V.ViTFeatures(bad, cfg, device="cpu")
    bad = {k: v for k, v in sd.items() if k != "blocks.0.attn.qkv.bias"}
    with pytest.raises(KeyError, match="blocks.0.attn.qkv.bias"):
        V.ViTFeatures(bad, cfg, device="cpu")
    with pytest.raises(NotImplementedError):
        V.ViTFeatures(sd, cfg, interpolation="bilinear", device="cpu")
    with pytest.raises(NotImplementedError):
        V.ViTFeatures(sd, dict(cfg, heads=4), device="cpu")   # head dim 32: no attention kernel
    m = V.ViTFeatures(dict(sd, **{"head.weight": torch.zeros(10, cfg["d"]), "head.bias": torch.zeros(10)}), cfg,
                      device="cpu")                          # a classifier head is ignored
    assert (m.T, m.npatch, m.d) == (10, 9, 128) and m.pos.shape == (9, 128) and m.row0.shape == (1, 128)
    assert torch.equal(m.row0[0], (sd["cls_token"][0, 0] + sd["pos_embed"][0, 0]).half())


def test_plan_descriptors(V):
    """Byte offsets of images packed back to back, shared tables for equal sizes, the tile height."""
    m = V.ViTFeatures(VR.make_state_dict(VR.SMALL, 0), VR.SMALL, device="cpu")
    desc, tab, rows = m.plan([(97, 61), (61, 97), (97, 61), (48, 48)])
    assert desc["src"].tolist() == [0, 3 * 97 * 61, 2 * 3 * 97 * 61, 3 * 3 * 97 * 61]
    assert desc[0].tolist()[3:] == desc[2].tolist()[3:] and desc[0].tolist()[3:] != desc[1].tolist()[3:]
    assert tab.dtype == torch.int32 and tab.numel() == m._tab_len
    # the tallest tile is the 97 -> 75 rows reduction's (scale s = 97 / 75, support 2 s): a patch row of 16
    # reads 16 s rows plus the support on both sides
    s = 97 / 75
    assert 16 * s <= rows <= 16 * s + 4 * s + 2
    n = tab.numel()
    m.plan([(61, 97)])
    assert m._tab_len == n                                   # every table was cached
    with pytest.raises(ValueError):
        m.plan([(0, 10)])


# ------------------------------------------------------------------------------------------ the tool's tables

def test_list_parsing_and_names(V, tmp_path):
    p = tmp_path / "train.txt"
    p.write_text("1000092795.jpg#0\tTwo young guys .\n  10002456.jpg  \n3.jpg#4#x\n")
    assert V.read_list(str(p)) == ["1000092795.jpg", "10002456.jpg", "3.jpg"]
    want = {"train": ("flickr30k-images", "train.txt", "train"), "val": ("flickr30k-images", "val.txt", "valid"),
            "test2016": ("flickr30k-images", "test_2016_flickr.txt", "test"),
            "test2017": ("test2017-images", "test_2017_flickr.txt", "test1"),
            "testcoco": ("testcoco-images", "test_2017_mscoco.txt", "test2")}
    for ds, (d, l, o) in want.items():
        assert V.dataset_paths("/data", ds) == (os.path.join("/data", d), os.path.join("/data", l), o)
    with pytest.raises(ValueError):
        V.dataset_paths("/data", "test2018")
