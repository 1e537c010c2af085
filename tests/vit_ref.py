"""CPU restatement of the ViT image feature extractor, for the tests of multimodal-s2ut_amd/vision.py.
Nothing here imports the product package, ``timm``, ``torchvision`` or ``transformers``.

Two parts.

The image transform in numpy: torchvision Resize(S, bicubic) on a PIL image, CenterCrop(S), ToTensor,
Normalize, and the patch rows of the patch-embedding GEMM.  The resample restates Pillow's 8-bit
Image.resize(BICUBIC) (Resample.c): per axis integer coefficients of 22 fractional bits from double
weights, a horizontal then a vertical pass, each pixel clamp((2^21 + sum pix k) >> 22, 0, 255).  It is
pinned bit for bit to Pillow's own results in tests/golden/vit_pillow_s48.npz (scripts/gen_vit_golden.py)
and, where PIL imports, to the live library.

timm's VisionTransformer.forward_features (num_classes=0) in torch: fp32 (or fp64 on double inputs) with
emulate=False, the reference every GPU result is compared with; emulate=True does the same arithmetic
but rounds through fp16 every weight and every tensor the product stores in fp16, at the places where
vision.py stores one.  Its distance from the fp32 restatement is the error floor a test's allowance is a
multiple of (TOL_FACTOR), the convention of tests/asr_ref.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F

TOL_FACTOR = 3.0            # allowance = TOL_FACTOR x the emulation's own max-abs distance
LN_EPS = 1e-6
BITS = 22

SMALL = dict(d=128, heads=2, mlp=256, layers=2, image_size=48, patch=16)
SMALL_224 = dict(d=128, heads=2, mlp=512, layers=1, image_size=224, patch=16)
WIDE = dict(d=768, heads=12, mlp=3072, layers=1, image_size=48, patch=16)
# the front end's S = 48 cases, (w, h): upscale with odd byte sizes, downscale with wide supports, no
# resample, a crop on one axis, an extreme aspect
SIZES_48 = [(97, 61), (61, 97), (200, 150), (150, 310), (48, 48), (50, 48), (48, 77), (31, 300)]
# the images of the HF golden: (w, h, seed)
GOLDEN_IMAGES = [(61, 97, 1), (200, 150, 2)]


# ------------------------------------------------------------------------------------------ images

def make_image(w, h, seed=0):
    """Seeded uint8 [h, w, 3]: a gradient under strong noise, clipped, so that runs of 0 and 255 sit next to
    mid-range pixels and the bicubic overshoot reaches both clamps."""
    g = np.random.default_rng([w, h, seed])
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 60 * np.sin(x / 7.0)[..., None] + 60 * np.cos(y / 5.0)[..., None] * np.array([1.0, -1.0, 0.5])
    return np.clip(np.round(base + g.normal(0, 90, (h, w, 3))), 0, 255).astype(np.uint8)


def resize_size(w, h, S):
    if min(w, h) == S:
        return w, h
    return (S, int(S * h / w)) if w <= h else (int(S * w / h), S)


def crop_origin(size, S):
    return int(round((size - S) / 2.0))


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coefficients(insize, outsize):
    """[(xmin, [int coefficient, ...]), ...] for every output index of one axis."""
    scale = insize / outsize
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    rows = []
    for xx in range(outsize):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = min(int(c + support + 0.5), insize)
        w, ww = [], 0.0
        for x in range(xmin, xmax):
            v = bicubic((x - c + 0.5) * ss)
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append((xmin, [int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS)) for v in w]))
    return rows


def resample_axis(img, outsize, axis):
    """One pass of the 8-bit resample along `axis` of uint8 [h, w, 3]."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((outsize,) + src.shape[1:], np.int64)
    for xx, (xmin, k) in enumerate(coefficients(src.shape[0], outsize)):
        kk = np.array(k, np.int64).reshape((-1,) + (1,) * (src.ndim - 1))
        out[xx] = ((1 << (BITS - 1)) + (src[xmin:xmin + len(k)] * kk).sum(0)) >> BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def pil_resize(img, w2, h2):
    """Image.resize((w2, h2), BICUBIC) of uint8 [h, w, 3]: horizontal pass, then vertical; an axis whose size
    does not change is not resampled."""
    h, w, _ = img.shape
    if w2 != w:
        img = resample_axis(img, w2, 1)
    if h2 != h:
        img = resample_axis(img, h2, 0)
    return img


def transform_u8(img, S):
    """Resize(S, bicubic) + CenterCrop(S) of uint8 [h, w, 3] -> uint8 [S, S, 3]."""
    h, w, _ = img.shape
    w2, h2 = resize_size(w, h, S)
    r = pil_resize(img, w2, h2)
    x0, y0 = crop_origin(w2, S), crop_origin(h2, S)
    return r[y0:y0 + S, x0:x0 + S]


def pillow_transform_u8(img, S):
    """The same through the live Pillow library."""
    from PIL import Image
    h, w, _ = img.shape
    w2, h2 = resize_size(w, h, S)
    im = Image.fromarray(img)
    if (w2, h2) != (w, h):
        im = im.resize((w2, h2), Image.BICUBIC)
    x0, y0 = crop_origin(w2, S), crop_origin(h2, S)
    return np.asarray(im.crop((x0, y0, x0 + S, y0 + S)))


def normalise(u8, mean=0.5, std=0.5):
    """ToTensor + Normalize as torch computes them: uint8 [S, S, 3] -> fp32 [3, S, S]."""
    x = torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).float() / 255
    return (x - mean) / std


def patchify(x, P):
    """[B, 3, S, S] -> [B, (S/P)^2, 3 P P], a patch's columns in (c, py, px) order, patches row-major."""
    B, C, S, _ = x.shape
    n = S // P
    return x.reshape(B, C, n, P, n, P).permute(0, 2, 4, 1, 3, 5).reshape(B, n * n, C * P * P)


def pixels(images, S):
    """uint8 images -> normalised fp32 [B, 3, S, S]."""
    return torch.stack([normalise(transform_u8(im, S)) for im in images])


# ------------------------------------------------------------------------------------------ the model

def make_state_dict(cfg, seed=0):
    """Seeded state dict under timm's key names; scales keep unit-variance tokens at roughly unit variance."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    d, Fd, P = cfg["d"], cfg["mlp"], cfg["patch"]
    T = (cfg["image_size"] // P) ** 2 + 1
    sd = {"cls_token": 0.5 * rn(1, 1, d), "pos_embed": 0.5 * rn(1, T, d),
          "patch_embed.proj.weight": rn(d, 3, P, P) / (3 * P * P) ** 0.5 * 2.0, "patch_embed.proj.bias": 0.1 * rn(d)}

    def ln(name):
        sd[name + ".weight"], sd[name + ".bias"] = 1.0 + 0.1 * rn(d), 0.1 * rn(d)

    def lin(name, nout, nin):
        sd[name + ".weight"], sd[name + ".bias"] = rn(nout, nin) / nin ** 0.5, 0.1 * rn(nout)

    for l in range(cfg["layers"]):
        p = f"blocks.{l}."
        ln(p + "norm1")
        lin(p + "attn.qkv", 3 * d, d)
        lin(p + "attn.proj", d, d)
        ln(p + "norm2")
        lin(p + "mlp.fc1", Fd, d)
        lin(p + "mlp.fc2", d, Fd)
    ln("norm")
    return sd


def checksums(sd):
    """{key: float64 [sum, sum of squares]} of a state dict: what the golden records of the weights."""
    return {k: np.array([float(v.double().sum()), float(v.double().pow(2).sum())]) for k, v in sd.items()}


def _q(emulate):
    return (lambda t: t.half().to(t.dtype)) if emulate else (lambda t: t)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(qkv, H, q):
    """[B, T, 3 d] = q | k | v -> [B, T, d], heads of d / H contiguous columns, scores scaled by hd^-0.5."""
    B, T, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    q_, k_, v_ = (qkv[..., i * d:(i + 1) * d].reshape(B, T, H, hd).transpose(1, 2) for i in range(3))
    P = torch.softmax(q_ @ k_.transpose(2, 3) * hd ** -0.5, dim=-1)
    return q((q(P) @ v_).transpose(1, 2).reshape(B, T, d))


def forward(sd, cfg, x, emulate=False):
    """Normalised pixels [B, 3, S, S] -> tokens [B, T, d], in the dtype of x (fp32 or fp64)."""
    q = _q(emulate)
    dt = x.dtype
    W = lambda n: q(sd[n + ".weight"].to(dt))
    Bi = lambda n: q(sd[n + ".bias"].to(dt))
    d, H, P = cfg["d"], cfg["heads"], cfg["patch"]
    ln = lambda t, n: q(F.layer_norm(t, (d,), W(n), Bi(n), LN_EPS))
    lin = lambda t, n: t @ W(n).t() + Bi(n)
    pos, cls = sd["pos_embed"].to(dt)[0], sd["cls_token"].to(dt)[0, 0]
    patches = patchify(q(x), P)
    emb = patches @ W("patch_embed.proj").reshape(d, -1).t() + Bi("patch_embed.proj")
    h = torch.cat([q(cls + pos[0]).expand(x.shape[0], 1, d), q(emb + q(pos[1:]))], 1)
    for l in range(cfg["layers"]):
        p = f"blocks.{l}."
        qkv = q(lin(ln(h, p + "norm1"), p + "attn.qkv"))
        h = q(h + lin(attention(qkv, H, q), p + "attn.proj"))
        z = q(lin(ln(h, p + "norm2"), p + "mlp.fc1"))
        h = q(h + lin(q(gelu(z)), p + "mlp.fc2"))
    return ln(h, "norm")


_CACHE = {}


def reference(name, cfg, seed, sizes):
    """(sd, images, fp32 tokens, emulated tokens) of a fixture: cfg, weight seed, ((w, h, image seed), ...);
    computed once per process and shared."""
    key = (name, seed, tuple(sizes))
    if key not in _CACHE:
        sd = make_state_dict(cfg, seed)
        images = [make_image(w, h, s) for w, h, s in sizes]
        x = pixels(images, cfg["image_size"])
        with torch.no_grad():
            _CACHE[key] = (sd, images, forward(sd, cfg, x), forward(sd, cfg, x, emulate=True))
    return _CACHE[key]
