"""GPU: the image front end (csrc/vision.hip) and the ViTFeatures forward built on it, against the CPU
restatement in tests/vit_ref.py.

The front end is integer arithmetic and a table lookup: it must equal the restatement (which is pinned to
Pillow, tests/test_vit.py) bit for bit.  The forward's allowance is measured, not chosen (the convention of
tests/test_gpu_units.py): a GPU result may be at most TOL_FACTOR (3) x as far from the fp32 restatement
(max-abs) as the restatement's own fp16-storage emulation is for the same inputs; every check prints its
floor and ratio."""
import os

import numpy as np
import pytest
import torch

import vit_ref as VR
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def V():
    return pkg("vision")


@pytest.fixture(scope="module")
def K():
    return pkg("kernels")


def _check(name, got, ref, emu):
    """got within TOL_FACTOR x the emulation's distance from the fp32 restatement -> the allowance."""
    floor = float((emu - ref).abs().max())
    err = float((got.float().cpu() - ref).abs().max())
    print(f"{name}: emulation floor {floor:.3e}, GPU error {err:.3e} ({err / floor if floor else float('nan'):.2f}x)")
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()
    assert floor > 0 and err <= VR.TOL_FACTOR * floor, (name, err, floor)
    return VR.TOL_FACTOR * floor


def _front(V, S, P):
    """A model whose only used parts are the front end's: image size S, patch P."""
    cfg = dict(VR.SMALL, image_size=S, patch=P, layers=0)
    return V.ViTFeatures(VR.make_state_dict(cfg, 0), cfg, device=DEV)


def _want(images, S, P):
    """The restatement's patch rows, fp16 [B, N, 3 P P]: torch's (u8 / 255 - 0.5) / 0.5 in fp32, rounded once."""
    return VR.patchify(VR.pixels(images, S), P).half()


# ------------------------------------------------------------------------------------------ front end

def test_front_end_bit_exact_s48(V):
    """One launch over all eight S = 48 cases; then each image alone, and the batch reversed."""
    m = _front(V, 48, 16)
    images = [VR.make_image(w, h, 0) for w, h in VR.SIZES_48]
    want = _want(images, 48, 16)
    got = m.patches(images).cpu()
    assert got.shape == want.shape == (8, 9, 768) and got.dtype == torch.float16
    for b, (w, h) in enumerate(VR.SIZES_48):
        n = int((got[b] != want[b]).sum())
        assert n == 0, f"{w}x{h}: {n} of {want[b].numel()} values differ"
    for b, im in enumerate(images):
        assert torch.equal(m.patches([im]).cpu()[0], got[b]), VR.SIZES_48[b]
    assert torch.equal(m.patches(images[::-1]).cpu(), got.flip(0))


def test_front_end_other_patch_size(V):
    m = _front(V, 32, 8)
    images = [VR.make_image(100, 60, 0), VR.make_image(45, 33, 1)]
    got = m.patches(images).cpu()
    assert got.shape == (2, 16, 192)
    assert torch.equal(got, _want(images, 32, 8))


def test_front_end_full_size(V):
    """500 x 375 -> 512 x 384 -> the 384 x 384 window, 576 patches."""
    m = _front(V, 384, 16)
    images = [VR.make_image(500, 375, 0)]
    got = m.patches(images).cpu()
    assert got.shape == (1, 576, 768)
    assert torch.equal(got, _want(images, 384, 16))


def test_front_end_normalisation_table(V):
    """Every uint8 value through the kernel (a 48 x 48 image is not resampled) against torch's arithmetic, with
    ImageNet's mean and std as well as the default."""
    im = np.zeros((48, 48, 3), np.uint8)
    im.reshape(-1)[:] = np.arange(48 * 48 * 3) % 256
    for mean, std in (((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))):
        cfg = dict(VR.SMALL, layers=0)
        m = V.ViTFeatures(VR.make_state_dict(cfg, 0), cfg, mean=mean, std=std, device=DEV)
        x = torch.from_numpy(im).permute(2, 0, 1).float() / 255
        want = ((x - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]).half()
        assert torch.equal(m.patches([im]).cpu(), VR.patchify(want[None], 16))


def test_front_end_refusals(V, K):
    m = _front(V, 48, 16)
    with pytest.raises(ValueError):
        m.patches([np.zeros((10, 10), np.uint8)])
    desc, tab, rows = m.plan([(3400, 3400)])                  # reduced 70 x: a patch reads > 1024 source rows
    assert rows * 16 * 3 > K.VISION_TILE_BYTES
    with pytest.raises(ValueError, match="LDS"):
        K.vision_patches(torch.zeros(8, dtype=torch.uint8, device=DEV), desc, tab, m.norm_tab, 48, 16, rows)
    desc, tab, rows = m.plan([(97, 61)])
    with pytest.raises(ValueError):                           # the image does not fit the buffer
        K.vision_patches(torch.zeros(100, dtype=torch.uint8, device=DEV), desc, tab, m.norm_tab, 48, 16, rows)


def test_nonfinite_rows(K):
    x = torch.randn(3, 5, 64).half().to(DEV)
    assert K.nonfinite_rows(x).tolist() == [0, 0, 0]
    x[1, 4, 63] = float("inf")
    x[2, 0, 0] = float("nan")
    assert K.nonfinite_rows(x).tolist() == [0, 1, 1]


# ------------------------------------------------------------------------------------------ forward

FORWARD = {
    "small_b1": (VR.SMALL, ((61, 97, 1),)),
    "small_b3": (VR.SMALL, ((61, 97, 1), (200, 150, 2), (48, 48, 3))),
    # 197 tokens: odd, and above the attention kernel's 128-key staging
    "small224_b2": (VR.SMALL_224, ((250, 230, 1), (224, 300, 2))),
    # the real widths of vit_base
    "wide_b2": (VR.WIDE, ((97, 61, 1), (50, 48, 2))),
}


@pytest.mark.parametrize("name", list(FORWARD))
def test_forward_matches_restatement(V, name):
    cfg, sizes = FORWARD[name]
    sd, images, ref, emu = VR.reference(name, cfg, 0, sizes)
    m = V.ViTFeatures(sd, cfg, device=DEV)
    got = m.forward_device(images)
    T = (cfg["image_size"] // cfg["patch"]) ** 2 + 1
    assert got.shape == (len(images), T, cfg["d"]) and got.dtype == torch.float16
    _check(f"vit {name}", got, ref, emu)
    # the assembly's offsets: the class token's row and the last patch's row by themselves
    _check(f"vit {name} token 0", got[:, 0], ref[:, 0], emu[:, 0])
    _check(f"vit {name} last token", got[:, T - 1], ref[:, T - 1], emu[:, T - 1])
    # the tokens before the blocks: X[b, 0] = cls + pos[0] exactly, X[b, 1 + i] = patch i + pos[1 + i]
    X = m.embed(m.patches(images)).float().cpu()
    row0 = (sd["cls_token"][0, 0] + sd["pos_embed"][0, 0]).half().float()
    assert torch.equal(X[:, 0], row0.expand(len(images), -1))
    x = VR.pixels(images, cfg["image_size"])
    W = sd["patch_embed.proj.weight"].reshape(cfg["d"], -1)
    emb = lambda q: q(VR.patchify(q(x), cfg["patch"]) @ q(W).t() + q(sd["patch_embed.proj.bias"]) + q(sd["pos_embed"][0, 1:]))
    _check(f"vit {name} patch tokens", X[:, 1:], emb(lambda t: t), emb(lambda t: t.half().float()))
    f = m.features(images)
    assert f.dtype == torch.float32 and not f.is_cuda and torch.equal(f, got.float().cpu())


# ------------------------------------------------------------------------------------------ end to end

def test_extract_dataset_end_to_end(V, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    cfg = VR.SMALL
    sd = VR.make_state_dict(cfg, 0)
    root = tmp_path / "multi30k"
    (root / "flickr30k-images").mkdir(parents=True)
    sizes = [(97, 61, 1), (61, 97, 2), (48, 48, 3), (150, 310, 4), (50, 48, 5)]
    names = [f"{i}.png" for i in range(len(sizes))]
    images = [VR.make_image(w, h, s) for w, h, s in sizes]
    for n, im in zip(names, images):
        Image.fromarray(im).save(str(root / "flickr30k-images" / n))
    (root / "val.txt").write_text("".join(f"{n}#0\ta caption\n" for n in names))
    ckpt = str(tmp_path / "vit.pth")
    torch.save({"state_dict": sd}, ckpt)
    m = V.ViTFeatures(V.load_checkpoint(ckpt), cfg, device=DEV)
    seen = []
    path, shape = V.extract_dataset(m, str(root), "val", str(tmp_path / "feats"), batch_size=2, num_workers=2,
                                    progress=lambda done, total: seen.append((done, total)))
    assert os.path.basename(path) == "valid.pth" and shape == (5, 10, 128) and seen == [(2, 5), (4, 5), (5, 5)]
    feats = pkg("manifest").ImageFeatures(str(tmp_path / "feats"), "valid")
    assert len(feats) == 5 and feats.feat.dtype == torch.float32
    direct = torch.cat([m.features(images[i:i + 2]) for i in range(0, 5, 2)])    # the tool's own batches
    for i in range(5):
        assert torch.equal(feats[i][0], direct[i]), i
    _, _, ref, emu = VR.reference("e2e", cfg, 0, tuple(sizes))
    _check("vit end to end", feats.feat, ref, emu)


def test_overflowing_checkpoint_raises(V):
    cfg = VR.SMALL
    sd = dict(VR.make_state_dict(cfg, 0))
    w = sd["blocks.0.mlp.fc2.weight"].clone()
    w[3, 5] = 1e6                                             # inf in fp16
    sd["blocks.0.mlp.fc2.weight"] = w
    m = V.ViTFeatures(sd, cfg, device=DEV)
    with pytest.raises(V.NonFiniteFeatures):
        m.features([VR.make_image(61, 97, 1), VR.make_image(48, 48, 2)])
