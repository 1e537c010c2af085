"""GPU: the attention-rollout kernels (csrc/rollout.hip) and ViTFeatures.rollout built on them, against the CPU
restatement in tests/rollout_ref.py (pinned to the reference's own function, tests/test_rollout.py).

Allowances are measured, not chosen.  Fused probabilities: TOL_FACTOR x the max-abs distance of the torch-fp32
evaluation of the same formula from float64, on the same fp16 qkv, floored at 4 fp32 ulps of 1.0 (4.8e-7: the
hardware exp is good to an ulp or two of values <= 1).  The discard is integer work: the result must equal the
restatement's.  Chain and exact route: TOL_FACTOR x the float32 restatement's distance from float64 on the same
matrices.  From pixels: TOL_FACTOR x the fp16-emulated restatement's distance from the float32 restatement; at a
discard ratio of 0.9 fp16 rounding moves entries across the threshold, the emulation takes flips of its own and
its distance contains them.  Every check prints its floor and its error."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import rollout_ref as RR
import vit_ref as VR
from conftest import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP4 = 4 * 2.0 ** -23


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


# ------------------------------------------------------------------------------------------ fused probabilities

# (H, hd, T): less than one tile; ragged tiles; 12 tiles + 5 with a non-power-of-two 1 / H; the WIDE config's
# head loop; the other head dims; the production T
PROB_SHAPES = [(2, 64, 10), (2, 64, 37), (3, 64, 197), (12, 64, 10), (2, 96, 37), (2, 128, 37), (2, 64, 577)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,hd,T", PROB_SHAPES)
def test_fused_probabilities(K, H, hd, T, B):
    gen = torch.Generator().manual_seed(1000 * T + 10 * H + B)
    qkv = (1.5 * torch.randn(B * T, 3 * H * hd, generator=gen)).half()
    A64 = RR.probabilities(qkv.double().view(B, T, -1), H)
    A32 = RR.probabilities(qkv.float().view(B, T, -1), H)
    dev = qkv.to(DEV)
    for fusion in RR.FUSIONS:
        want = RR.fuse(A64, fusion)
        floor = float((RR.fuse(A32, fusion).double() - want).abs().max())
        allow = max(RR.TOL_FACTOR * floor, ULP4)
        got = K.rollout_probs(dev, B, H, T, fusion)
        assert got.shape == (B, T, T) and got.dtype == torch.float32
        err = float((got.cpu().double() - want).abs().max())
        print(f"probs H {H} hd {hd} T {T} B {B} {fusion}: torch fp32 vs fp64 {floor:.2e}, allowance {allow:.2e}, "
              f"kernel vs fp64 {err:.2e}")
        assert torch.isfinite(got).all() and err <= allow, (fusion, err, allow)
        assert torch.equal(K.rollout_probs(dev, B, H, T, fusion), got)             # every run: the same bits
        # into layer 1 of a [B, 2, T, T] workspace: the batch stride, and nothing outside the matrices is touched
        ws = torch.full((B, 2, T, T), -1.0, device=DEV)
        K.rollout_probs(dev, B, H, T, fusion, out=ws[:, 1])
        assert torch.equal(ws[:, 1], got) and bool((ws[:, 0] == -1.0).all())


def test_fused_probabilities_refusals(K):
    with pytest.raises(NotImplementedError, match="limit"):
        K.rollout_probs(torch.zeros(K.ROLLOUT_MAX_T + 1, 384, dtype=torch.float16, device=DEV), 1, 2, K.ROLLOUT_MAX_T + 1)
    with pytest.raises(NotImplementedError, match="head dim"):
        K.rollout_probs(torch.zeros(10, 192, dtype=torch.float16, device=DEV), 1, 2, 10)
    with pytest.raises(ValueError, match="head_fusion"):
        K.rollout_probs(torch.zeros(10, 384, dtype=torch.float16, device=DEV), 1, 2, 10, "median")


# ------------------------------------------------------------------------------------------ discard

def _discard_case(K, x, k):
    """x fp32 [..., T, T] on the host: the kernel's result must equal the restatement's, matrix by matrix --
    the same zeroed set, the survivors untouched -- twice."""
    T = x.shape[-1]
    want = torch.stack([RR.discard(m, k) for m in x.reshape(-1, T, T)]).view_as(x)
    got = K.rollout_discard(x.to(DEV).clone(), k)
    assert torch.equal((got == 0).cpu(), want == 0), f"zeroed sets differ in {int(((got.cpu() == 0) != (want == 0)).sum())} places"
    assert torch.equal(got.cpu(), want)
    assert torch.equal(K.rollout_discard(x.to(DEV).clone(), k), got)
    return got


@pytest.mark.parametrize("seed", range(len(RR.STACKS)))
def test_discard_seeded_stacks(K, seed):
    T, H, L = RR.STACKS[seed]
    A = RR.attention_stack(T, H, L, seed)
    x = torch.stack([RR.fuse(A, f) for f in RR.FUSIONS])            # [3, L, T, T]: 3 L matrices in one launch
    for ratio in RR.RATIOS:
        _discard_case(K, x, RR.discard_count(T, ratio))


def test_discard_production_size(K):
    T = 577
    x = torch.softmax(2.0 * torch.randn(T, T, generator=torch.Generator().manual_seed(5)), dim=-1)
    assert RR.discard_count(T, 0.9) == 299636
    got = _discard_case(K, x, 299636)
    assert int((got == 0).sum()) == 299636 - (1 if float(x[0, 0]) <= float(x.reshape(-1).kthvalue(299636).values) else 0)


def test_discard_ties_and_index0(K):
    same = torch.full((4, 4), 0.25)
    for k in (0, 1, 5, 15, 16):
        _discard_case(K, same, k)
    Fm = torch.arange(16, dtype=torch.float32).flip(0).reshape(4, 4) + 1
    _discard_case(K, Fm, 3)
    Fm[0, 0] = 0.0                                                   # index 0 among the k smallest
    for k in (1, 3, 16):
        _discard_case(K, Fm, k)
    # many ties at the boundary, over several blocks of the ordered scan, and exact zeros below it
    g = torch.Generator().manual_seed(9)
    coarse = (torch.rand(2, 3, 37, 37, generator=g) * 8).floor() / 8
    for k in (0, 1, 100, 171, 685, 1232, 1368, 1369):
        _discard_case(K, coarse, k)
    coarse577 = (torch.rand(577, 577, generator=g) * 4).floor() / 4
    _discard_case(K, coarse577, 299636)
    _discard_case(K, torch.rand(1, 1, generator=g), 1)              # T = 1: only index 0, kept


def test_discard_nonfinite_input_stays_in_bounds(K):
    """inf and NaN are large keys: whatever they select, nothing is indexed outside the matrix (the guard rows
    around it stay) and every run gives the same bits."""
    x = torch.rand(3, 37, 37, generator=torch.Generator().manual_seed(2))
    x[1, 3, 5], x[1, 7, 7], x[1, 0, 1] = float("inf"), float("nan"), float("nan")
    x[1, 0, 0] = 2.0                                                 # index 0 is not among the k smallest
    d = x.to(DEV)
    a = K.rollout_discard(d[1:2].clone(), 1232)
    assert torch.equal(K.rollout_discard(d[1:2].clone(), 1232).view(torch.int32), a.view(torch.int32))
    assert int((a == 0).sum()) == 1232 and bool(torch.isinf(a[0, 3, 5])) and bool(torch.isnan(a[0, 7, 7]))
    with pytest.raises(ValueError):
        K.rollout_discard(d, 37 * 37 + 1)


# ------------------------------------------------------------------------------------------ normalise and chain

def _chain_case(K, name, a, normalization):
    """a fp32 [B, L, T, T] on the host."""
    mask, bad = K.rollout_chain(a.to(DEV), normalization)
    assert bad.tolist() == [0] * a.shape[0] and mask.shape == (a.shape[0], a.shape[2] - 1)
    for b in range(a.shape[0]):
        want = RR.chain(a[b], normalization, torch.float64)
        floor = float((RR.chain(a[b], normalization, torch.float32).double() - want).abs().max())
        err = float((mask[b].cpu().double() - want).abs().max())
        print(f"chain {name} image {b} {normalization}: restatement fp32 vs fp64 {floor:.2e}, kernel vs fp64 {err:.2e}")
        assert err <= RR.TOL_FACTOR * floor, (name, b, normalization, err, floor)
    again, _ = K.rollout_chain(a.to(DEV), normalization)
    assert torch.equal(again, mask)
    return mask


@pytest.mark.parametrize("normalization", ["reference", "row"])
@pytest.mark.parametrize("seed", [1, 2])
def test_chain_seeded_stacks(K, seed, normalization):
    T, H, L = RR.STACKS[seed]
    A = RR.attention_stack(T, H, L, seed)
    k = RR.discard_count(T, 0.9)
    a = torch.stack([torch.stack([RR.discard(m, k) for m in RR.fuse(A, f)]) for f in RR.FUSIONS])
    _chain_case(K, f"T {T} ratio 0.9", a, normalization)
    _chain_case(K, f"T {T} ratio 0", torch.stack([RR.fuse(A, f) for f in RR.FUSIONS]), normalization)


def test_chain_production_size(K):
    T, L = 577, 3
    A = torch.softmax(2.0 * torch.randn(L, T, T, generator=torch.Generator().manual_seed(6)), dim=-1)
    a = torch.stack([RR.discard(m, 299636) for m in A])[None]
    for normalization in ("reference", "row"):
        _chain_case(K, "T 577", a, normalization)


def test_chain_empty_and_nonfinite_are_flagged(K):
    T = 10
    ok = RR.attention_stack(T, 1, 2, 4)[:, 0]
    empty = torch.eye(T).expand(2, T, T)                             # the class token attends to itself alone
    nan = ok.clone()
    nan[1, 0, 3] = float("nan")
    mask, bad = K.rollout_chain(torch.stack([ok, empty, nan]).contiguous().to(DEV))
    assert bad.tolist() == [0, 1, 1]
    assert not mask[1:].any() and torch.isfinite(mask).all() and float(mask[0].max()) == 1.0


# ------------------------------------------------------------------------------------------ end to end

S96 = dict(VR.SMALL, image_size=96, layers=3)
S224 = dict(VR.SMALL_224, layers=2)
E2E = {
    "s96_l3": (S96, ((120, 100, 1), (96, 130, 2), (300, 200, 3))),
    "s224_l2": (S224, ((250, 230, 1), (224, 300, 2))),
    "s224_l2_pre_norm": (dict(S224, pre_norm=True, mean=(0.48145466, 0.4578275, 0.40821073),
                              std=(0.26862954, 0.26130258, 0.27577711)), ((250, 230, 1), (224, 300, 2))),
}


@pytest.mark.parametrize("name", list(E2E))
def test_rollout_exact_route(V, name):
    """The restatement on the product's own fused matrices: no threshold flips between the two."""
    cfg, sizes = E2E[name]
    sd, images, _ = RR.reference(name, cfg, 0, sizes)
    m = V.ViTFeatures(sd, cfg, device=DEV)
    plain = m.forward_device(images)
    for fusion, ratio, normalization in (("mean", 0.9, "reference"), ("max", 0.9, "row"), ("min", 0.5, "reference"),
                                         ("mean", 0.0, "reference")):
        mask, bad, Y, fused = m.rollout_device(images, fusion, ratio, normalization, keep_fused=True)
        assert torch.equal(Y, plain)                                 # the features of the same forward
        assert bad.tolist() == [0] * len(images) and fused.shape == (len(images), cfg["layers"], m.T, m.T)
        fused = fused.cpu()
        for b in range(len(images)):
            want = RR.rollout_fused(fused[b], ratio, normalization, torch.float64)
            floor = float((RR.rollout_fused(fused[b], ratio, normalization, torch.float32).double() - want).abs().max())
            err = float((mask[b].cpu().double() - want).abs().max())
            print(f"exact {name} image {b} {fusion} {ratio} {normalization}: restatement fp32 vs fp64 {floor:.2e}, "
                  f"GPU vs fp64 {err:.2e}")
            assert err <= RR.TOL_FACTOR * floor, (name, b, fusion, ratio, err, floor)
        host = m.rollout(images, fusion, ratio, normalization)
        n = cfg["image_size"] // cfg["patch"]
        assert host.shape == (len(images), n, n) and host.dtype == torch.float32 and not host.is_cuda
        assert torch.equal(host.view(len(images), -1), mask.cpu())


@pytest.mark.parametrize("ratio", [0.0, 0.9])
@pytest.mark.parametrize("name", list(E2E))
def test_rollout_from_pixels(V, name, ratio):
    cfg, sizes = E2E[name]
    sd, images, _ = RR.reference(name, cfg, 0, sizes)
    ref32, emu = RR.from_pixels(name, cfg, 0, sizes, "mean", ratio, "reference")
    got = V.ViTFeatures(sd, cfg, device=DEV).rollout(images, "mean", ratio, "reference")
    floor = float((emu - ref32).abs().max())
    err = float((got.view(len(images), -1) - ref32).abs().max())
    print(f"from pixels {name} ratio {ratio}: fp16 emulation vs fp32 {floor:.2e}, bound {RR.TOL_FACTOR * floor:.2e}, "
          f"GPU vs fp32 {err:.2e}")
    assert torch.isfinite(got).all() and floor > 0 and err <= RR.TOL_FACTOR * floor, (name, ratio, err, floor)


def test_rollout_chunks_and_empty_raise(V, monkeypatch):
    cfg, sizes = E2E["s96_l3"]
    sd, images, _ = RR.reference("s96_l3", cfg, 0, sizes)
    m = V.ViTFeatures(sd, cfg, device=DEV)
    parts = torch.cat([m.rollout(images[:2]), m.rollout(images[2:])])
    monkeypatch.setattr(V, "ROLLOUT_WS_BYTES", 2 * 4 * 3 * 37 * 37)  # two images per pass
    assert m.rollout_chunk() == 2
    assert torch.equal(m.rollout(images), parts)
    with pytest.raises(ValueError, match="per pass"):
        m.rollout_device(images)
    with pytest.raises(V.EmptyRollout, match="image 0"):             # everything but [0, 0] discarded
        m.rollout(images, discard_ratio=1.0)


def test_pre_norm_features_match_clip_golden(V):
    gold = np.load(os.path.join(GOLDEN, "rollout_clip_small.npz"))
    cfg = RR.CLIP_SMALL
    sd = RR.make_state_dict(cfg, 0)
    images = [VR.make_image(w, h, s) for w, h, s in RR.CLIP_IMAGES]
    x = RR.pixels(images, cfg["image_size"])
    with torch.no_grad():
        emu = RR.forward(sd, cfg, x, emulate=True)[0]
    ref = torch.from_numpy(gold["out32"])
    got = V.ViTFeatures(sd, cfg, device=DEV).forward_device(images)
    floor = float((emu - ref).abs().max())
    err = float((got.float().cpu() - ref).abs().max())
    print(f"pre-norm features vs HF CLIPVisionModel fp32: emulation floor {floor:.3e}, GPU error {err:.3e}")
    assert got.shape == ref.shape and torch.isfinite(got).all() and floor > 0 and err <= VR.TOL_FACTOR * floor


def test_cli_end_to_end(V, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    spec = importlib.util.spec_from_file_location("mms2ut_vit_rollout", os.path.join(ROOT, "scripts", "mms2ut_vit_rollout.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = V.model_config("vit_tiny_patch16_384")
    ckpt = str(tmp_path / "vit_tiny.pth")
    torch.save({"state_dict": VR.make_state_dict(cfg, 0)}, ckpt)
    sizes = [(97, 61, 1), (61, 97, 2), (48, 48, 3)]
    paths = []
    for i, (w, h, s) in enumerate(sizes):
        paths.append(str(tmp_path / f"im{i}.png"))
        Image.fromarray(VR.make_image(w, h, s)).save(paths[-1])
    rc = cli.main(["--image", *paths, "--model", "vit_tiny_patch16_384", "--checkpoint-path", ckpt, "--save-dir",
                   str(tmp_path / "out"), "--overlay-dir", str(tmp_path / "png"), "--batch-size", "2", "--num-workers", "2",
                   "--device", DEV])
    assert rc == 0
    masks = torch.load(str(tmp_path / "out" / "images_rollout.pth"))
    assert masks.shape == (3, 24, 24) and masks.dtype == torch.float32 and torch.isfinite(masks).all()
    assert masks.view(3, -1).max(dim=1).values.tolist() == [1.0, 1.0, 1.0] and float(masks.min()) >= 0.0
    with Image.open(str(tmp_path / "png" / "im1_rollout.png")) as im:
        assert im.size == (61, 97) and im.mode == "RGB"
    assert sorted(os.listdir(str(tmp_path / "png"))) == ["im0_rollout.png", "im1_rollout.png", "im2_rollout.png"]
