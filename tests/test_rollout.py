"""CPU: the rollout restatement (tests/rollout_ref.py) against the reference's own function and against the
``transformers`` library's CLIPVisionModel (tests/golden/rollout_reference.npz, rollout_clip_small.npz, written
by scripts/gen_rollout_golden.py), and the host side of ViTFeatures.rollout: the tie and index-0 rules of the
discard on constructed matrices, the pre-norm model table, the tool's argument errors and the overlay.

Allowances are measured, not chosen: the reference computes in fp32, so the restatement's float64 run may be
TOL_FACTOR x as far from a golden mask as the restatement's own float32 run is from its float64 run."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import rollout_ref as RR
import vit_ref as VR
from conftest import GOLDEN, ROOT, pkg


@pytest.fixture(scope="module")
def V():
    return pkg("vision")


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("mms2ut_vit_rollout", os.path.join(ROOT, "scripts", "mms2ut_vit_rollout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------ reference golden

@pytest.mark.parametrize("seed", range(len(RR.STACKS)))
def test_restatement_matches_reference_golden(seed):
    gold = np.load(os.path.join(GOLDEN, "rollout_reference.npz"))
    T, H, L = RR.STACKS[seed]
    A = RR.attention_stack(T, H, L, seed)
    have = np.array([float(A.double().sum()), float(A.double().pow(2).sum())])
    assert np.allclose(have, gold[f"sum_{T}"], rtol=1e-9), "the seeded stack drifted from the golden's; regenerate"
    n = int((T - 1) ** 0.5)
    for fusion in RR.FUSIONS:
        for ratio in RR.RATIOS:
            want = torch.from_numpy(gold[f"mask_{T}_{fusion}_{ratio}"]).double()
            assert want.shape == (n, n)
            k = RR.discard_count(T, ratio)
            assert min(RR.tie_gap(RR.fuse(A[l], fusion), k) for l in range(L)) > 0        # no tie: topk is defined
            m64 = RR.grid(RR.rollout(A, fusion, ratio, "reference", torch.float64))
            m32 = RR.grid(RR.rollout(A, fusion, ratio, "reference", torch.float32)).double()
            floor, err = float((m32 - m64).abs().max()), float((m64 - want).abs().max())
            print(f"T {T} {fusion} ratio {ratio}: restatement fp32 vs fp64 {floor:.2e}, fp64 vs the reference {err:.2e}")
            # T = 5 at 0.9 keeps 3 of 25 entries: the mask is exactly one-hot in every precision (floor 0, error 0)
            assert err <= RR.TOL_FACTOR * floor and (floor > 0 or T == 5), (fusion, ratio, err, floor)
            # after a discard the rows no longer sum to one and the row normalisation is another function: the
            # reference's quirk is not a rounding matter (at ratio 0 every s_i is 1 and the two coincide)
            if T > 5 and ratio == 0.9:
                row = RR.grid(RR.rollout(A, fusion, ratio, "row", torch.float64))
                assert float((row - want).abs().max()) > 1e-3


def test_clip_restatement_matches_hf_golden():
    gold = np.load(os.path.join(GOLDEN, "rollout_clip_small.npz"))
    cfg = RR.CLIP_SMALL
    sd = RR.make_state_dict(cfg, 0)
    assert "patch_embed.proj.bias" not in sd and "norm_pre.weight" in sd
    want = {k[4:]: gold[k] for k in gold.files if k.startswith("sum_")}
    assert sorted(want) == sorted(sd)                       # nothing missing, nothing unexpected
    have = VR.checksums(sd)
    drift = [k for k in want if not np.allclose(have[k], want[k], rtol=1e-9, atol=1e-12)]
    assert not drift, f"the seeded weights drifted from the golden's ({drift[:3]}...); regenerate. Not a parity failure."
    x = RR.pixels([VR.make_image(w, h, s) for w, h, s in RR.CLIP_IMAGES], cfg["image_size"])
    assert np.allclose([float(x.double().sum()), float(x.double().pow(2).sum())], gold["pix_sum"], rtol=1e-9)
    with torch.no_grad():
        tok, _, probs = RR.forward({k: v.double() for k, v in sd.items()}, cfg, x.double())
    out32, out64 = torch.from_numpy(gold["out32"]).double(), torch.from_numpy(gold["out64"])
    att32, att64 = torch.from_numpy(gold["att32"]).double(), torch.from_numpy(gold["att64"])
    noise, att_noise = float(gold["noise"]), float(gold["att_noise"])
    assert tok.shape == out32.shape == (2, 10, 128) and att64.shape == (2, 2, 2, 10, 10)
    assert noise == float((out32 - out64).abs().max()) > 0 and att_noise == float((att32 - att64).abs().max()) > 0
    err = float((tok - out32).abs().max())
    aerr = float((torch.stack(probs) - att32).abs().max())
    print(f"pre-norm restatement (fp64) vs HF fp32: tokens {err:.2e} (HF fp32 vs double {noise:.2e}), probabilities "
          f"{aerr:.2e} (HF {att_noise:.2e}); vs HF double {float((tok - out64).abs().max()):.2e}")
    assert err <= VR.TOL_FACTOR * noise and aerr <= VR.TOL_FACTOR * att_noise
    # without the switch the same weights give something else
    with torch.no_grad():
        plain, _, _ = RR.forward({k: v.double() for k, v in sd.items()}, dict(cfg, pre_norm=False), x.double())
    assert float((plain - out64).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------ the discard's rules

def _zeroed(Fm, k):
    return sorted(RR.discard_indices(Fm, k).tolist())


def test_discard_tie_and_index0_rules():
    T = 4
    same = torch.full((T, T), 0.25)
    assert _zeroed(same, 5) == [1, 2, 3, 4]                  # all equal: flat order, index 0 counted but kept
    assert _zeroed(same, 0) == [] and _zeroed(same, 16) == list(range(1, 16))
    Fm = torch.arange(16, dtype=torch.float32).flip(0).reshape(T, T) + 1     # index 0 holds the largest value
    assert _zeroed(Fm, 3) == [13, 14, 15] and _zeroed(Fm, 16) == list(range(1, 16))
    Fm[0, 0] = 0.0                                           # index 0 among the k smallest: k - 1 entries go
    assert _zeroed(Fm, 3) == [14, 15]
    out = RR.discard(Fm, 3)
    assert out[0, 0] == 0.0 and out.reshape(-1)[14:].tolist() == [0.0, 0.0] and torch.equal(out.reshape(-1)[1:14], Fm.reshape(-1)[1:14])
    tie = torch.tensor([[0.5, 0.1, 0.3], [0.1, 0.3, 0.1], [0.3, 0.1, 0.9]])
    assert _zeroed(tie, 3) == [1, 3, 5] and _zeroed(tie, 5) == [1, 2, 3, 5, 7] and _zeroed(tie, 6) == [1, 2, 3, 4, 5, 7]
    assert RR.tie_gap(tie, 3) == 0.0 and RR.tie_gap(tie, 4) > 0
    assert [RR.discard_count(t, 0.9) for t in (5, 37, 197, 577)] == [22, 1232, 34928, 299636]


def test_normalisations_and_empty_rollout():
    a = torch.stack([RR.discard(f, 10) for f in RR.attention_stack(5, 1, 2, 3)[:, 0]])
    ref, row = RR.chain(a, "reference"), RR.chain(a, "row")
    assert float(ref.max()) == 1.0 == float(row.max()) and float((ref - row).abs().max()) > 1e-3
    # "row" is the textbook rollout: rows of every a_l sum to one, so do the product's
    eye = torch.eye(5, dtype=torch.float64)
    R = eye
    for l in range(2):
        m = (a[l].double() + eye) / 2
        R = (m / m.sum(-1, keepdim=True)) @ R
    assert torch.allclose(R.sum(-1), torch.ones(5, dtype=torch.float64)) and torch.allclose(row, R[0, 1:] / R[0, 1:].max())
    with pytest.raises(ValueError):
        RR.chain(torch.eye(5)[None])                         # the class token attends to itself alone
    with pytest.raises(ValueError):
        RR.chain(torch.full((1, 5, 5), float("nan")))


# ------------------------------------------------------------------------------------------ host side

def test_pre_norm_model_table(V):
    c = V.model_config("vit_base_patch16_clip_384.laion2b_ft_in12k_in1k")
    assert (c["d"], c["heads"], c["layers"], c["mlp"], c["image_size"], c["patch"], c["pre_norm"]) == (768, 12, 12, 3072, 384, 16, True)
    assert c["mean"] == (0.48145466, 0.4578275, 0.40821073) and c["std"] == (0.26862954, 0.26130258, 0.27577711)
    assert "pre_norm" not in V.model_config("vit_base_patch16_384")
    with pytest.raises(ValueError, match="vit_huge_patch14_224"):
        V.model_config("vit_huge_patch14_224")
    with pytest.raises(NotImplementedError, match="vit_base_patch16_clip_224.openai.*QuickGELU"):
        V.model_config("vit_base_patch16_clip_224.openai")


def test_pre_norm_constructor(V):
    cfg = RR.CLIP_SMALL
    sd = RR.make_state_dict(cfg, 0)
    m = V.ViTFeatures(sd, cfg, device="cpu")
    assert m.pre_norm and not m.patch_b.any() and torch.equal(m.pre_g, sd["norm_pre.weight"].half())
    assert torch.equal(m.norm_tab, V.norm_table((0.5,) * 3, (0.5,) * 3))
    clip = V.ViTFeatures(sd, dict(cfg, mean=V.CLIP_MEAN, std=V.CLIP_STD), device="cpu")
    assert torch.equal(clip.norm_tab, V.norm_table(V.CLIP_MEAN, V.CLIP_STD))
    with pytest.raises(KeyError, match="norm_pre.weight"):
        V.ViTFeatures({k: v for k, v in sd.items() if k != "norm_pre.weight"}, cfg, device="cpu")
    with pytest.raises(KeyError, match="patch_embed.proj.bias"):      # a plain model still needs its bias
        V.ViTFeatures(sd, VR.SMALL, device="cpu")
    plain = V.ViTFeatures(VR.make_state_dict(VR.SMALL, 0), VR.SMALL, device="cpu")
    assert not plain.pre_norm and plain.rollout_chunk() == (256 << 20) // (4 * 2 * 100)


def test_rollout_argument_errors(V):
    m = V.ViTFeatures(VR.make_state_dict(VR.SMALL, 0), VR.SMALL, device="cpu")
    im = [VR.make_image(48, 48, 0)]
    with pytest.raises(ValueError, match="head_fusion"):
        m.rollout(im, head_fusion="median")
    with pytest.raises(ValueError, match="normalization"):
        m.rollout(im, normalization="column")
    with pytest.raises(ValueError, match="discard_ratio"):
        m.rollout(im, discard_ratio=1.5)
    assert m.rollout([]).shape == (0, 3, 3)


def test_cli_argument_errors(cli, capsys):
    base = ["--model", "vit_tiny_patch16_384", "--checkpoint-path", "x.pth", "--save-dir", "out"]
    for extra, text in (([], "either --dataset"), (["--dataset", "val"], "--path"),
                        (["--dataset", "val", "--path", "p", "--image", "a.png"], "either --dataset"),
                        (["--image", "a.png", "--discard-ratio", "1.2"], "--discard-ratio"),
                        (["--image", "a.png", "--head-fusion", "median"], "--head-fusion"),
                        (["--image", "a.png", "--normalization", "col"], "--normalization"),
                        (["--image", "a.png", "--batch-size", "0"], "--batch-size")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    for name, text in (("vit_base_patch32_384", "is not supported"), ("vit_base_patch16_clip_224.openai", "QuickGELU")):
        with pytest.raises(SystemExit) as e:
            cli.main(["--model", name, "--checkpoint-path", "x.pth", "--save-dir", "out", "--image", "a.png"])
        assert e.value.code == 2 and text in capsys.readouterr().err


def test_overlay_size_and_determinism(V):
    pytest.importorskip("PIL")
    im = VR.make_image(97, 61, 4)
    mask = torch.rand(3, 3, generator=torch.Generator().manual_seed(0)).numpy()
    mask = mask / mask.max()
    a, b = V.overlay(im, mask), V.overlay(im, mask)
    assert a.shape == im.shape == (61, 97, 3) and a.dtype == np.uint8 and np.array_equal(a, b)
    assert np.array_equal(V.overlay(im, np.zeros((3, 3))), im)            # an empty mask leaves the image
    hot = V.overlay(im, np.ones((3, 3)), alpha=1.0)
    assert (hot[..., 0] == 255).all() and not hot[..., 1:].any()
