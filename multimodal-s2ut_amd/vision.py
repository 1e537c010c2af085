"""ViT image features from raw images: what the reference's scripts/extract_feature/get_img_feat_vit.py
computes with timm (``vit_*_patch16_384``, ``num_classes=0``, ``forward_features``) and writes as the
``{split}.pth`` fp32 [N, 577, d] that manifest.ImageFeatures loads.

Forward only.  The image front end -- timm's eval transform: torchvision Resize(S, bicubic) on the PIL
image, CenterCrop(S), ToTensor, Normalize(mean = std = 0.5) -- runs on the device in one launch per batch
(csrc/vision.hip): Pillow's 8-bit bicubic resample bit for bit from coefficient tables computed here in
double, the crop, the normalisation as a table lookup, and the patch rows.  The patch embedding is one
batched NT GEMM whose epilogue adds pos_embed[1:] and writes at token offset 1 (the class rows are one
strided copy); the blocks are encoders.transformer_layers, the pre-LN layer loop the wav2vec2 encoder runs,
at eps 1e-6.  The checked getter and the layer dictionary are encoders.py's too.

``timm``, ``torchvision`` and ``transformers`` are not dependencies: the semantics are restated here and
in tests/vit_ref.py; the checkpoint's key names and tensor shapes pin the loader."""
import concurrent.futures as cf
import math
import os
import sys

import numpy as np
import torch

from . import _lib
from . import kernels as K
from .encoders import TIMM_LAYER, Weights, layer_dict, read_safetensors, transformer_layers

LN_EPS = 1e-6                   # timm's VisionTransformer: partial(nn.LayerNorm, eps=1e-6)
PRECISION_BITS = 22             # Pillow's 8-bit resample: 32 - 8 - 2
# model name -> (width, heads, depth); patch 16, image 384, MLP ratio 4
MODELS = {"vit_tiny_patch16_384": (192, 3, 12), "vit_small_patch16_384": (384, 6, 12),
          "vit_base_patch16_384": (768, 12, 12), "vit_large_patch16_384": (1024, 16, 24)}
# --dataset -> (image directory without "-images", list file, output name)
DATASETS = {"train": ("flickr30k", "train.txt", "train"), "val": ("flickr30k", "val.txt", "valid"),
            "test2016": ("flickr30k", "test_2016_flickr.txt", "test"),
            "test2017": ("test2017", "test_2017_flickr.txt", "test1"),
            "testcoco": ("testcoco", "test_2017_mscoco.txt", "test2")}
TABLE_CACHE_INTS = 16 << 20     # the device coefficient tables are dropped and rebuilt past 64 MiB
# timm's CLIP-style ViTs (vision_transformer.py, pre_norm=True, no patch bias): norm_pre after the position
# embeddings; their pretrained cfgs carry the OpenAI-CLIP mean and std.  name -> (width, heads, depth)
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
PRE_NORM_MODELS = {"vit_base_patch16_clip_384": (768, 12, 12),
                   "vit_base_patch16_clip_384.laion2b_ft_in12k_in1k": (768, 12, 12)}
# the rollout's per-layer matrices [chunk, layers, T, T] fp32 never exceed this; a batch is cut into chunks
ROLLOUT_WS_BYTES = 256 << 20


class NonFiniteFeatures(RuntimeError):
    """An image's features hold inf or NaN (fp16 activations overflowed): nothing is written."""


class EmptyRollout(RuntimeError):
    """An image's rollout reaches no patch (its maximum is 0) or holds inf or NaN: nothing is written."""


def model_config(name):
    """{d, heads, layers, mlp, image_size, patch} of a timm model name; the CLIP-style models add pre_norm,
    mean and std."""
    if name in PRE_NORM_MODELS:
        d, H, L = PRE_NORM_MODELS[name]
        return {"d": d, "heads": H, "layers": L, "mlp": 4 * d, "image_size": 384, "patch": 16, "pre_norm": True,
                "mean": CLIP_MEAN, "std": CLIP_STD}
    if "clip" in name and (name.endswith(".openai") or "quickgelu" in name):
        raise NotImplementedError(f"model '{name}' uses QuickGELU, which is not supported (only erf-GELU)")
    if name not in MODELS:
        raise ValueError(f"model '{name}' is not supported (one of {', '.join(sorted({**MODELS, **PRE_NORM_MODELS}))})")
    d, H, L = MODELS[name]
    return {"d": d, "heads": H, "layers": L, "mlp": 4 * d, "image_size": 384, "patch": 16}


# ------------------------------------------------------------------------------------------ transform

def resize_size(w, h, S):
    """torchvision Resize(S) on a (w, h) image: the short side becomes S, the long side int(S * long / short)."""
    if min(w, h) == S:
        return w, h
    return (S, int(S * h / w)) if w <= h else (int(S * w / h), S)


def crop_origin(size, S):
    """torchvision CenterCrop's origin along one axis (Python's round: half to even)."""
    return int(round((size - S) / 2.0))


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def resample_rows(insize, outsize, lo, n):
    """Rows lo .. lo + n of Pillow's coefficient table for an 8-bit bicubic resample of one axis from insize
    to outsize (Resample.c precompute_coeffs + normalize_coeffs_8bpc, in double as there): -> (first int32 [n],
    taps int32 [n], coef int32 [n, ksize]); output index lo + i is clamp((2^21 + sum_t pix[first[i] + t] *
    coef[i, t]) >> 22).  insize == outsize: Pillow skips the pass; the table is the identity."""
    if insize == outsize:
        return (np.arange(lo, lo + n, dtype=np.int32), np.ones(n, np.int32),
                np.full((n, 1), 1 << PRECISION_BITS, np.int32))
    scale = insize / outsize
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    first, taps, coef = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, ksize), np.int32)
    for i in range(n):
        center = (lo + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), insize) - xmin
        w = _bicubic((np.arange(xmax) + xmin - center + 0.5) * ss)
        ww = np.cumsum(w)[-1]                        # Pillow's running sum, in index order
        if ww != 0.0:
            w = w / ww
        first[i], taps[i] = xmin, xmax
        coef[i, :xmax] = np.trunc(np.where(w < 0, -0.5, 0.5) + w * (1 << PRECISION_BITS)).astype(np.int32)
    return first, taps, coef


def norm_table(mean, std):
    """fp16 [3, 256]: ToTensor + Normalize of every uint8 as torch computes it, (u8 / 255 - mean) / std in
    fp32, rounded to fp16 once."""
    u = torch.arange(256, dtype=torch.float32) / 255
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    if m.numel() != 3 or s.numel() != 3 or not bool((s != 0).all()):
        raise ValueError("mean and std must have three entries, std non-zero")
    return ((u[None, :] - m[:, None]) / s[:, None]).half()


# ------------------------------------------------------------------------------------------ checkpoints

def load_checkpoint(path):
    """timm-layout state dict of a file: safetensors (in-tree reader) or a torch.save'd state dict, also
    wrapped in ``state_dict`` or ``model``."""
    if path.endswith(".safetensors"):
        return read_safetensors(path)
    if path.endswith(".npz"):
        raise NotImplementedError(f"{path}: timm's .npz checkpoints are not supported")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    for key in ("state_dict", "model"):
        if isinstance(sd, dict) and key in sd and isinstance(sd[key], dict):
            sd = sd[key]
    if not isinstance(sd, dict) or not all(isinstance(v, torch.Tensor) for v in sd.values()):
        raise ValueError(f"{path}: not a state dict (nor one wrapped in 'state_dict' or 'model')")
    return sd


class ViTFeatures:
    """timm VisionTransformer.forward_features (num_classes=0: every token after the final norm) on raw
    RGB images, with timm's eval transform in front."""

    def __init__(self, state_dict, config, mean=None, std=None, interpolation="bicubic", device="cuda"):
        if interpolation != "bicubic":
            raise NotImplementedError(f"interpolation '{interpolation}' is not supported (only \"bicubic\")")
        c = self.cfg = dict(config)
        # the transform's mean and std: the arguments, else the config's (pre-norm models), else timm's 0.5
        mean = c.get("mean", (0.5, 0.5, 0.5)) if mean is None else mean
        std = c.get("std", (0.5, 0.5, 0.5)) if std is None else std
        self.pre_norm = bool(c.get("pre_norm", False))
        self.device = dev = torch.device(device)
        d, H, Fd, S, P = c["d"], c["heads"], c["mlp"], c["image_size"], c["patch"]
        if d % H or d // H not in K.FLASH_HD:
            raise NotImplementedError(f"ViT head dim {d}/{H} is not supported (the attention kernel has {K.FLASH_HD})")
        if S % P or (3 * P * P) % 8 or d % 8 or Fd % 8:
            raise ValueError(f"ViT config: patch {P} must divide image size {S}; 3 P P, d and mlp must be multiples of 8")
        self.d, self.H, self.S, self.P = d, H, S, P
        self.npatch = (S // P) ** 2
        self.T = T = self.npatch + 1
        w = Weights(state_dict, "ViT checkpoint", device,
                    hints={"pos_embed": " (position embeddings are not interpolated to other image sizes)"})
        get, f16 = w.get, w.f16
        self.patch_w = f16(get("patch_embed.proj.weight", (d, 3, P, P)).reshape(d, 3 * P * P))
        if self.pre_norm and "patch_embed.proj.bias" not in state_dict:      # timm: bias = not pre_norm
            self.patch_b = torch.zeros(d, dtype=K.F16, device=dev)
        else:
            self.patch_b = f16(get("patch_embed.proj.bias", (d,)))
        if self.pre_norm:
            self.pre_g, self.pre_b = f16(get("norm_pre.weight", (d,))), f16(get("norm_pre.bias", (d,)))
        pos, cls = get("pos_embed", (1, T, d))[0], get("cls_token", (1, 1, d))[0, 0]
        self.row0 = f16((cls + pos[0]).reshape(1, d))            # the class token's row, rounded once
        self.pos = f16(pos[1:])
        self.layers = [layer_dict(w, f"blocks.{l}.", d, Fd, TIMM_LAYER) for l in range(c["layers"])]
        self.norm_g, self.norm_b = f16(get("norm.weight", (d,))), f16(get("norm.bias", (d,)))
        self.norm_tab = norm_table(mean, std).contiguous().to(dev)
        self._tab_off, self._tab_host, self._tab_len, self._tab_dev = {}, [], 0, None
        self._host = None                                        # pinned fp16 staging of features()

    @classmethod
    def from_checkpoint(cls, model_name, checkpoint_path, device="cuda", **kw):
        return cls(load_checkpoint(checkpoint_path), model_config(model_name), device=device, **kw)

    # ---------------------------------------------------------------------------------- front end

    def _axis(self, insize, outsize, lo):
        """(bounds offset, coefficient offset, coefficients per row, most source rows one patch reads) of an
        axis' table in the device buffer; computed once per (insize, outsize)."""
        key = (insize, outsize, lo)
        if key not in self._tab_off:
            first, taps, coef = resample_rows(insize, outsize, lo, self.S)
            P = self.P
            span = int(max(int((first[i:i + P] + taps[i:i + P]).max()) - int(first[i:i + P].min())
                           for i in range(0, self.S, P)))
            b0 = self._tab_len
            self._tab_host += [np.stack([first, taps], 1).reshape(-1), coef.reshape(-1)]
            self._tab_off[key] = (b0, b0 + 2 * self.S, coef.shape[1], span)
            self._tab_len += 2 * self.S + coef.size
            self._tab_dev = None
        return self._tab_off[key]

    def plan(self, sizes):
        """Descriptors (host, byte offsets of images packed back to back), the device table and the tile
        height of a batch of (w, h) images."""
        if self._tab_len > TABLE_CACHE_INTS:
            self._tab_off, self._tab_host, self._tab_len, self._tab_dev = {}, [], 0, None
        desc = np.zeros(len(sizes), np.dtype(_lib.ImageDesc))
        off, rows, S = 0, 1, self.S
        for b, (w, h) in enumerate(sizes):
            if w < 1 or h < 1 or max(w, h) > K.VISION_MAX_SIDE:
                raise ValueError(f"image {b} of the batch: size {w}x{h} is not supported")
            w2, h2 = resize_size(w, h, S)
            hb, hk, hn, _ = self._axis(w, w2, crop_origin(w2, S))
            vb, vk, vn, span = self._axis(h, h2, crop_origin(h2, S))
            desc[b] = (off, w, h, hb, hk, hn, vb, vk, vn)
            off += 3 * w * h
            rows = max(rows, span)
        if self._tab_dev is None:
            self._tab_dev = torch.from_numpy(np.concatenate(self._tab_host).astype(np.int32)).to(self.device)
        return desc, self._tab_dev, rows

    def patches(self, images):
        """uint8 numpy [h, w, 3] images -> fp16 [B, (S/P)^2, 3 P P] on the device: the transform and patchify."""
        arrs = []
        for i, a in enumerate(images):
            a = np.asarray(a)
            if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
                raise ValueError(f"image {i} of the batch: uint8 [h, w, 3] expected, got {a.dtype} {a.shape}")
            arrs.append(np.ascontiguousarray(a))
        desc, tab, rows = self.plan([(a.shape[1], a.shape[0]) for a in arrs])
        total = sum(a.size for a in arrs)
        buf = torch.empty(total, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        view, off = buf.numpy(), 0
        for a in arrs:
            view[off:off + a.size] = a.reshape(-1)
            off += a.size
        return K.vision_patches(buf.to(self.device, non_blocking=True), desc, tab, self.norm_tab, self.S, self.P, rows)

    # ---------------------------------------------------------------------------------- forward

    def embed(self, patches):
        """fp16 patch rows [B, N, 3 P P] -> fp16 tokens [B, N + 1, d]: X[b, 0] = cls + pos[0]; X[b, 1 + i] =
        patch-embed(patch i) + bias + pos[1 + i], the sum in the batched GEMM's epilogue."""
        B, N, Kd = patches.shape
        d, T = self.d, self.T
        X = torch.empty(B, T, d, dtype=K.F16, device=patches.device)
        K.gemm(patches, self.patch_w, X[:, 1:], N, d, Kd, lda=Kd, ldb=Kd, ldc=d, batch=B, sA=(N * Kd, 0), sC=(T * d, 0),
               epi=K.EPI_DROP_RESID, bias=self.patch_b, aux=self.pos, ldaux=d)
        K.copy2d(self.row0.expand(B, d), X[:, 0], B, d)
        if self.pre_norm:
            X = K.layernorm(X.view(B * T, d), self.pre_g, self.pre_b, LN_EPS)[0].view(B, T, d)
        return X

    def tokens(self, X, on_qkv=None):
        """fp16 [B, T, d] -> fp16 [B, T, d]: the blocks and the final norm."""
        B, T, d = X.shape
        Y = transformer_layers(X, self.layers, self.H, LN_EPS, on_qkv=on_qkv)
        return K.layernorm(Y, self.norm_g, self.norm_b, LN_EPS)[0].view(B, T, d)

    def forward_device(self, images):
        return self.tokens(self.embed(self.patches(images)))

    # ---------------------------------------------------------------------------------- rollout

    def rollout_chunk(self):
        """Images one rollout pass may hold: its [chunk, layers, T, T] fp32 workspace stays within
        ROLLOUT_WS_BYTES (at least one image)."""
        return max(1, ROLLOUT_WS_BYTES // (4 * max(len(self.layers), 1) * self.T * self.T))

    def rollout_device(self, images, head_fusion="mean", discard_ratio=0.9, normalization="reference", keep_fused=False):
        """One chunk (at most rollout_chunk() images) on the device -> (mask fp32 [B, T - 1], bad int32 [B],
        features fp16 [B, T, d] of the same forward, the fused matrices before the discard fp32 [B, L, T, T] if
        keep_fused else None).  Each layer's head-fused probabilities are formed from the qkv buffer the
        attention kernel reads, straight into the workspace; then one discard and one chain launch."""
        B, T, L = len(images), self.T, len(self.layers)
        if head_fusion not in K.ROLLOUT_FUSIONS:
            raise ValueError(f"head_fusion '{head_fusion}' (one of {', '.join(K.ROLLOUT_FUSIONS)})")
        if normalization not in K.ROLLOUT_NORMALIZATIONS:
            raise ValueError(f"normalization '{normalization}' (one of {', '.join(K.ROLLOUT_NORMALIZATIONS)})")
        k = K.rollout_discard_count(T, discard_ratio)
        if T > K.ROLLOUT_MAX_T:
            raise NotImplementedError(f"rollout: {T} tokens exceed the kernels' limit of {K.ROLLOUT_MAX_T}")
        if L < 1 or not 1 <= B <= self.rollout_chunk():
            raise ValueError(f"rollout: 1 .. {self.rollout_chunk()} images per pass and at least one layer expected")
        ws = torch.empty(B, L, T, T, dtype=torch.float32, device=self.device)
        Y = self.tokens(self.embed(self.patches(images)),
                        on_qkv=lambda l, qkv: K.rollout_probs(qkv, B, self.H, T, head_fusion, out=ws[:, l]))
        fused = ws.clone() if keep_fused else None
        K.rollout_discard(ws, k)
        mask, bad = K.rollout_chain(ws, normalization)
        return mask, bad, Y, fused

    def rollout(self, images, head_fusion="mean", discard_ratio=0.9, normalization="reference"):
        """Attention rollout of each image, as the reference's vit_rollout.py computes it for a batch of one
        -> host fp32 [B, S/P, S/P], each map divided by its maximum.  normalization "reference" divides
        column j by the sum of row j (the reference's a / a.sum(-1)); "row" divides each row by its own sum.
        The batch is processed rollout_chunk() images at a time."""
        images = list(images)
        n = self.S // self.P
        out = torch.empty(len(images), n, n, dtype=torch.float32)
        step = self.rollout_chunk()
        for i in range(0, len(images), step):
            mask, bad, _, _ = self.rollout_device(images[i:i + step], head_fusion, discard_ratio, normalization)
            mask, bad = mask.cpu(), bad.cpu()
            for b, flag in enumerate(bad.tolist()):
                if flag:
                    raise EmptyRollout(f"image {i + b} of the batch: the rollout is empty or non-finite; nothing written")
            out[i:i + mask.shape[0]] = mask.view(-1, n, n)
        return out

    def features(self, images, out=None):
        """fp32 [B, T, d] on the host (into out, if given): fp16 over PCIe into a pinned buffer kept between
        calls, widened (exactly) straight into the destination."""
        Y = self.forward_device(images)
        B = Y.shape[0]
        bad = K.nonfinite_rows(Y)
        if self._host is None or self._host.shape[0] < B:
            self._host = torch.empty(B, self.T, self.d, dtype=K.F16, pin_memory=True)
        host = self._host[:B]
        host.copy_(Y, non_blocking=True)
        bad = bad.cpu()
        torch.cuda.current_stream(self.device).synchronize()
        for b, flag in enumerate(bad.tolist()):
            if flag:
                raise NonFiniteFeatures(f"image {b} of the batch: non-finite features (the fp16 activations "
                                        "overflowed); nothing written")
        if out is None:
            return host.float()
        if tuple(out.shape) != (B, self.T, self.d) or out.dtype != torch.float32 or out.is_cuda:
            raise ValueError(f"features: out must be a host fp32 tensor of shape {(B, self.T, self.d)}")
        return out.copy_(host)


# ------------------------------------------------------------------------------------------ the tool

def read_list(path):
    """File names of a Multi30k image list: the text before the first '#' of every line, stripped."""
    with open(path) as f:
        return [line.strip().split("#")[0] for line in f]


def dataset_paths(root, dataset):
    """(image directory, list file, output name) of --dataset under --path."""
    if dataset not in DATASETS:
        raise ValueError(f"dataset '{dataset}' (one of {', '.join(DATASETS)})")
    images, listing, out = DATASETS[dataset]
    return os.path.join(root, images + "-images"), os.path.join(root, listing), out


def decode_image(path):
    """RGB uint8 [h, w, 3] of an image file; no EXIF rotation, as the reference."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def extract_files(model, paths, batch_size=32, num_workers=8, progress=None):
    """fp32 [N, T, d] features of image files, in order.  A pool of num_workers threads decodes batch
    i + 1 while the device works on batch i."""
    if batch_size < 1 or num_workers < 1:
        raise ValueError("batch_size and num_workers must be >= 1")
    paths = list(paths)
    out = torch.empty(len(paths), model.T, model.d, dtype=torch.float32)
    batches = [paths[i:i + batch_size] for i in range(0, len(paths), batch_size)]
    with cf.ThreadPoolExecutor(max_workers=num_workers) as pool:
        pending = [pool.submit(decode_image, p) for p in batches[0]] if batches else []
        done = 0
        for i, _ in enumerate(batches):
            images = [f.result() for f in pending]
            pending = [pool.submit(decode_image, p) for p in batches[i + 1]] if i + 1 < len(batches) else []
            model.features(images, out=out[done:done + len(images)])
            done += len(images)
            if progress:
                progress(done, len(paths))
    return out


def extract_dataset(model, root, dataset, save_dir, batch_size=32, num_workers=8, progress=None):
    """The reference's tool: the images of a Multi30k split -> {save_dir}/{name}.pth fp32 [N, T, d]."""
    image_dir, listing, name = dataset_paths(root, dataset)
    files = read_list(listing)
    feats = extract_files(model, [os.path.join(image_dir, f) for f in files], batch_size, num_workers, progress)
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, name + ".pth")
    torch.save(feats, path)
    return path, tuple(feats.shape)


def overlay(image, mask, alpha=0.6):
    """Presentation only, on the host: uint8 [h, w, 3] image with the rollout mask [n, n] (values in [0, 1])
    resized to it (PIL bilinear) and blended over it towards red, weight alpha * mask -> uint8 [h, w, 3]."""
    from PIL import Image
    image = np.asarray(image)
    h, w, _ = image.shape
    m8 = np.clip(np.rint(np.asarray(mask, dtype=np.float64) * 255.0), 0, 255).astype(np.uint8)
    m = np.asarray(Image.fromarray(m8).resize((w, h), Image.BILINEAR), dtype=np.float64)[..., None] * (alpha / 255.0)
    heat = np.array([255.0, 0.0, 0.0])
    return np.clip(np.rint(image * (1.0 - m) + heat * m), 0, 255).astype(np.uint8)


def rollout_files(model, paths, batch_size=8, num_workers=8, head_fusion="mean", discard_ratio=0.9,
                  normalization="reference", overlay_dir=None, progress=None):
    """fp32 [N, S/P, S/P] rollout masks of image files, in order, decoded on a thread pool as extract_files
    does.  overlay_dir: also one PNG per image there, {file's base name}_rollout.png, the overlay()."""
    if batch_size < 1 or num_workers < 1:
        raise ValueError("batch_size and num_workers must be >= 1")
    paths = list(paths)
    n = model.S // model.P
    out = torch.empty(len(paths), n, n, dtype=torch.float32)
    batches = [paths[i:i + batch_size] for i in range(0, len(paths), batch_size)]
    if overlay_dir:
        from PIL import Image
        os.makedirs(overlay_dir, exist_ok=True)
    with cf.ThreadPoolExecutor(max_workers=num_workers) as pool:
        pending = [pool.submit(decode_image, p) for p in batches[0]] if batches else []
        done = 0
        for i, batch in enumerate(batches):
            images = [f.result() for f in pending]
            pending = [pool.submit(decode_image, p) for p in batches[i + 1]] if i + 1 < len(batches) else []
            out[done:done + len(images)] = model.rollout(images, head_fusion, discard_ratio, normalization)
            if overlay_dir:
                for j, (p, im) in enumerate(zip(batch, images)):
                    name = os.path.splitext(os.path.basename(p))[0] + "_rollout.png"
                    Image.fromarray(overlay(im, out[done + j].numpy())).save(os.path.join(overlay_dir, name))
            done += len(images)
            if progress:
                progress(done, len(paths))
    return out


def print_progress(done, total):
    print(f"images {done}/{total}", file=sys.stderr, flush=True)
