"""Unit vocoder: fairseq's CodeHiFiGAN (unit_hifigan_*_dur) forward on the HIP kernels of
csrc/vocoder.hip -- the third stage of the reference pipeline (3_generate_waveform.sh,
generate_waveform_from_code.py --vocoder --vocoder-cfg --dur-prediction).

Forward only, one utterance at a time as fairseq does.  Activations are time-major fp16 [T, C]; every
convolution is one launch with its activation, bias, residual and the 1/nk stage average fused
(kernels.conv1d_tm / conv_transpose1d_tm), the duration predictor runs in fp32.  Weight norm is
folded and the weights are repacked into the kernels' layout once, at load."""
import ctypes as C
import json
import os
import wave as _wave

import numpy as np
import torch

from . import _lib
from . import kernels as K

LRELU_SLOPE = 0.1          # fairseq hifigan.LRELU_SLOPE
POST_SLOPE = 0.01          # F.leaky_relu's default, in front of conv_post
UNIT_OFFSET = 4            # <s> <pad> </s> <unk> precede the units in the dictionary
CONFIG_DEFAULTS = {"resblock": "1", "model_in_dim": 128, "num_embeddings": 1000, "embedding_dim": 128}


def parse_config(cfg):
    """Validated copy of a CodeHiFiGAN config.json dict (the keys the generator reads)."""
    c = dict(CONFIG_DEFAULTS)
    c.update(cfg)
    for key in ("multispkr", "f0", "embedder_params"):
        if c.get(key):
            raise NotImplementedError(f"CodeHiFiGAN config '{key}' is not supported (single-speaker unit vocoder only)")
    if str(c["resblock"]) != "1":
        raise NotImplementedError(f"CodeHiFiGAN resblock '{c['resblock']}' is not supported (only \"1\")")
    for key in ("upsample_rates", "upsample_kernel_sizes", "upsample_initial_channel", "resblock_kernel_sizes",
                "resblock_dilation_sizes"):
        if key not in c:
            raise ValueError(f"CodeHiFiGAN config: '{key}' is missing")
    if len(c["upsample_rates"]) != len(c["upsample_kernel_sizes"]):
        raise ValueError("CodeHiFiGAN config: upsample_rates and upsample_kernel_sizes differ in length")
    if len(c["resblock_kernel_sizes"]) != len(c["resblock_dilation_sizes"]):
        raise ValueError("CodeHiFiGAN config: resblock_kernel_sizes and resblock_dilation_sizes differ in length")
    if c["model_in_dim"] != c["embedding_dim"]:
        raise NotImplementedError("CodeHiFiGAN model_in_dim != embedding_dim (speaker / f0 inputs) is not supported")
    if any(k % 2 == 0 for k in c["resblock_kernel_sizes"]):
        raise ValueError("CodeHiFiGAN config: resblock kernel sizes must be odd")
    dp = c.get("dur_predictor_params")
    if dp:
        for key in ("encoder_embed_dim", "var_pred_hidden_dim", "var_pred_kernel_size"):
            if key not in dp:
                raise ValueError(f"CodeHiFiGAN dur_predictor_params: '{key}' is missing")
        if dp["var_pred_kernel_size"] != 3:
            # the second conv pads by 1 whatever the kernel size: other sizes change the length
            raise NotImplementedError("duration predictor kernel sizes other than 3 are not supported")
        if dp["encoder_embed_dim"] != c["embedding_dim"]:
            raise ValueError("CodeHiFiGAN dur_predictor_params: encoder_embed_dim != embedding_dim")
    return c


def fold_weight_norm(sd):
    """State dict with every weight-normed pair folded into a plain ``*.weight``: w = g v / |v|, the
    norm over all dims but dim 0 (the input-channel dim of a ConvTranspose1d weight).  Accepts
    ``weight_g / weight_v`` and ``parametrizations.weight.original0 / original1`` keys."""
    out = {}
    for key, v in sd.items():
        if key.endswith(".weight_g") or key.endswith(".parametrizations.weight.original0"):
            continue
        if key.endswith(".weight_v"):
            base, g = key[:-len(".weight_v")], sd[key[:-len("_v")] + "_g"]
        elif key.endswith(".parametrizations.weight.original1"):
            base, g = key[:-len(".parametrizations.weight.original1")], sd[key[:-1] + "0"]
        else:
            out[key] = v
            continue
        v32 = v.float()
        norm = v32.reshape(v32.shape[0], -1).norm(dim=1).view(-1, *([1] * (v32.dim() - 1)))
        out[base + ".weight"] = v32 * (g.float() / norm)
    return out


def pack_conv_weight(W):
    """Conv1d weight [Cout, Cin, k] -> the fp16 image mms2ut_conv1d_tm reads (include/mms2ut.h)."""
    Cout, Cin, k = W.shape
    CoutP = K.round_up(Cout, 16)
    parts = []
    for c0 in range(0, Cin, _lib.VOC_CIN_CHUNK):
        cw = min(_lib.VOC_CIN_CHUNK, Cin - c0)
        steps = -(-k * cw // 32)
        P = torch.zeros(CoutP, steps * 32, dtype=torch.float32)
        P[:Cout, :k * cw] = W[:, c0:c0 + cw, :].float().permute(0, 2, 1).reshape(Cout, k * cw)
        parts.append(P.view(CoutP, steps, 32).permute(1, 0, 2))
    return torch.cat(parts, 0).contiguous().half().reshape(-1)


def pack_conv_transpose_weight(W, stride):
    """ConvTranspose1d weight [Cin, Cout, k] -> `stride` polyphase images for mms2ut_conv_transpose1d_tm."""
    Cin, Cout, k = W.shape
    taps = -(-k // stride)
    out = []
    for r in range(stride):
        Wr = torch.zeros(Cout, Cin, taps, dtype=torch.float32)
        for m in range(taps):
            j = r + (taps - 1 - m) * stride
            if j < k:
                Wr[:, :, m] = W[:, :, j].float().t()
        out.append(pack_conv_weight(Wr))
    return torch.cat(out)


def units_from_tokens(tokens):
    """Hypothesis tokens -> unit codes: dictionary index n + 4 is code n; eos and the specials drop."""
    t = torch.as_tensor(tokens, dtype=torch.long).reshape(-1)
    return t[t >= UNIT_OFFSET] - UNIT_OFFSET


def read_code_file(path):
    """--in-code-file: one utterance per line, space-separated ints -> list of lists."""
    out = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            try:
                out.append([int(t) for t in line.split()])
            except ValueError:
                raise ValueError(f"{path}:{n}: not a line of integer unit codes") from None
    return out


def write_wav(path, wave, sr=16000):
    """fp32 waveform in [-1, 1] -> 16-bit mono PCM WAV (stdlib wave; samples round(x * 32767), clipped)."""
    x = wave.detach().float().cpu().numpy() if torch.is_tensor(wave) else np.asarray(wave, dtype=np.float32)
    s = np.clip(np.round(x.astype(np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with _wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(s.tobytes())


class _Conv:
    __slots__ = ("w", "b", "cout", "k", "dil")

    def __init__(self, w, b, cout, k, dil=1):
        self.w, self.b, self.cout, self.k, self.dil = w, b, cout, k, dil


class CodeHiFiGAN:
    """fairseq CodeHiFiGAN (CodeGenerator + optional VariancePredictor) in eval mode."""

    def __init__(self, state_dict, cfg, device="cuda"):
        self.cfg = c = parse_config(cfg)
        self.device = torch.device(device)
        sd = fold_weight_norm(state_dict)
        dev = self.device

        def want(name, t, shape):
            # the kernels trust these shapes: the packed images are sized by them
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name} has shape {tuple(t.shape)}, the config implies {tuple(shape)}")

        def conv(name, cout, cin, k, dil=1):
            W = sd[name + ".weight"]
            want(name + ".weight", W, (cout, cin, k))
            want(name + ".bias", sd[name + ".bias"], (cout,))
            return _Conv(pack_conv_weight(W).to(dev), sd[name + ".bias"].float().contiguous().to(dev), W.shape[0],
                         W.shape[2], dil)

        E = sd["dict.weight"].float()
        if tuple(E.shape) != (c["num_embeddings"], c["embedding_dim"]):
            raise ValueError(f"dict.weight {tuple(E.shape)} does not match the config")
        self.dict16 = E.half().contiguous().to(dev)
        ch = c["upsample_initial_channel"]
        self.pre = conv("conv_pre", ch, c["model_in_dim"], 7)
        self.ups, self.stages = [], []
        nk = len(c["resblock_kernel_sizes"])
        for i, (u, k) in enumerate(zip(c["upsample_rates"], c["upsample_kernel_sizes"])):
            W = sd[f"ups.{i}.weight"]                      # [Cin, Cout, k]
            want(f"ups.{i}.weight", W, (ch, ch // 2, k))
            want(f"ups.{i}.bias", sd[f"ups.{i}.bias"], (ch // 2,))
            ch //= 2
            self.ups.append((pack_conv_transpose_weight(W, u).to(dev), sd[f"ups.{i}.bias"].float().contiguous().to(dev),
                             W.shape[1], k, u))
            blocks = []
            for j, (rk, dils) in enumerate(zip(c["resblock_kernel_sizes"], c["resblock_dilation_sizes"])):
                n = i * nk + j
                blocks.append([(conv(f"resblocks.{n}.convs1.{m}", ch, ch, rk, d), conv(f"resblocks.{n}.convs2.{m}", ch, ch, rk))
                               for m, d in enumerate(dils)])
            self.stages.append(blocks)
        Wp = sd["conv_post.weight"].float()                # [1, Cin, k]
        want("conv_post.weight", Wp, (1, ch, 7))
        self.post_w = Wp[0].t().contiguous().to(dev)       # [k, Cin]
        self.post_b = float(sd["conv_post.bias"].float()[0])
        self.post_pad = (Wp.shape[2] - 1) // 2
        self.dur = None
        if c.get("dur_predictor_params"):
            dp = c["dur_predictor_params"]
            Hd, Ed, kd = dp["var_pred_hidden_dim"], dp["encoder_embed_dim"], dp["var_pred_kernel_size"]
            for name, shape in (("conv1.0.weight", (Hd, Ed, kd)), ("conv2.0.weight", (Hd, Hd, kd)), ("proj.weight", (1, Hd)),
                                ("proj.bias", (1,))) + tuple((n, (Hd,)) for n in ("conv1.0.bias", "conv2.0.bias", "ln1.weight",
                                                                                 "ln1.bias", "ln2.weight", "ln2.bias")):
                want("dur_predictor." + name, sd["dur_predictor." + name], shape)
            f = lambda n: sd["dur_predictor." + n].float().contiguous().to(dev)
            self.dur = {
                "dict32": E.contiguous().to(dev),
                "w1": sd["dur_predictor.conv1.0.weight"].float().permute(2, 1, 0).contiguous().to(dev),   # [k, Cin, Cout]
                "b1": f("conv1.0.bias"), "g1": f("ln1.weight"), "be1": f("ln1.bias"),
                "w2": sd["dur_predictor.conv2.0.weight"].float().permute(2, 1, 0).contiguous().to(dev),
                "b2": f("conv2.0.bias"), "g2": f("ln2.weight"), "be2": f("ln2.bias"),
                "pw": f("proj.weight").reshape(-1), "pb": float(sd["dur_predictor.proj.bias"].float()[0]),
            }
        self.launches = 0      # kernel launches of the last synthesize() call
        self._desc = self._describe()

    def _describe(self):
        """mms2ut_hifigan for mms2ut_hifigan_fwd: pointers into the tensors this object keeps alive."""
        c = self.cfg
        dils = c["resblock_dilation_sizes"]
        if len(self.ups) > _lib.VOC_MAX_STAGES or len(dils) > _lib.VOC_MAX_RESBLOCKS or \
                max(len(d) for d in dils) > _lib.VOC_MAX_DILS:
            raise NotImplementedError(f"CodeHiFiGAN with more than {_lib.VOC_MAX_STAGES} stages, "
                                      f"{_lib.VOC_MAX_RESBLOCKS} ResBlocks per stage or {_lib.VOC_MAX_DILS} dilations")
        m = _lib.HifiGan()
        m.dict, m.n_embed, m.D = self.dict16.data_ptr(), self.dict16.shape[0], self.dict16.shape[1]
        m.C0, m.n_stages, m.nk = self.pre.cout, len(self.ups), len(dils)
        for j, d in enumerate(dils):
            m.nd[j] = len(d)

        def put(dst, cv):
            dst.w, dst.b, dst.k, dst.dil = cv.w.data_ptr(), cv.b.data_ptr(), cv.k, cv.dil

        put(m.pre, self.pre)
        for i, ((uw, ub, ch, k, u), blocks) in enumerate(zip(self.ups, self.stages)):
            up = m.ups[i]
            up.w, up.b, up.k, up.u, up.cout = uw.data_ptr(), ub.data_ptr(), k, u, ch
            for j, block in enumerate(blocks):
                for d, (c1, c2) in enumerate(block):
                    put(m.c1[i][j][d], c1)
                    put(m.c2[i][j][d], c2)
        m.post_w, m.post_b, m.post_k = self.post_w.data_ptr(), self.post_b, self.post_w.shape[0]
        m.slope, m.post_slope = LRELU_SLOPE, POST_SLOPE
        return m

    @classmethod
    def from_files(cls, ckpt, cfg_json, device="cuda"):
        with open(cfg_json) as f:
            cfg = json.load(f)
        sd = torch.load(ckpt, map_location="cpu", weights_only=True)["generator"]
        return cls(sd, cfg, device)

    def _codes(self, codes):
        c = torch.as_tensor(codes, dtype=torch.long).reshape(-1).to(self.device).contiguous()
        if c.numel() == 0:
            raise ValueError("CodeHiFiGAN: empty unit sequence")
        return c

    def durations(self, codes):
        """(logd fp32 [T], dur int32 [T]) of the duration predictor, on the device."""
        if self.dur is None:
            raise ValueError("this vocoder has no duration predictor (config without dur_predictor_params)")
        d = self.dur
        h = K.var_pred_layer(d["dict32"], d["w1"], d["b1"], d["g1"], d["be1"], idx=self._codes(codes))
        return K.var_pred_layer(h, d["w2"], d["b2"], d["g2"], d["be2"], proj=(d["pw"], d["pb"]))

    def _frames(self, codes, dur_prediction):
        """-> (codes on the device, inclusive prefix sum of the durations or None, rows after the repeat)."""
        codes = self._codes(codes)
        if int(codes.min()) < 0 or int(codes.max()) >= self.dict16.shape[0]:
            raise ValueError(f"unit code outside [0, {self.dict16.shape[0]})")
        if not dur_prediction:
            return codes, None, codes.numel()
        cum = torch.cumsum(self.durations(codes)[1].long(), 0)
        return codes, cum, int(cum[-1])

    def synthesize(self, codes, dur_prediction=False):
        """Unit codes [T] -> fp32 waveform [T_out] on the device (16 kHz for the released models).  The
        generator's launches are issued by one library call (mms2ut_hifigan_fwd)."""
        codes, cum, frames = self._frames(codes, dur_prediction)
        ws_halves, T_wave, n = C.c_int64(0), C.c_int64(0), C.c_int(0)
        desc = C.byref(self._desc)
        _lib.call("mms2ut_hifigan_sizes", desc, frames, C.byref(ws_halves), C.byref(T_wave))
        ws = torch.empty(ws_halves.value, dtype=torch.float16, device=self.device)
        wave = torch.empty(T_wave.value, dtype=torch.float32, device=self.device)
        _lib.call("mms2ut_hifigan_fwd", desc, codes.data_ptr(), codes.numel(), K._p(cum), frames, ws.data_ptr(),
                  wave.data_ptr(), C.byref(n), K._s())
        self.launches = n.value + (2 if dur_prediction else 0)
        return wave

    def synthesize_stepwise(self, codes, dur_prediction=False):
        """The same forward with one library call per kernel (kernels.conv1d_tm, ...): what
        mms2ut_hifigan_fwd issues, spelled out.  Bit-identical to synthesize(); for tests and for
        looking at intermediate tensors."""
        codes, cum, T_out = self._frames(codes, dur_prediction)
        n = 2 if dur_prediction else 0
        x = K.embed_repeat(self.dict16, codes, cum, T_out)
        p = self.pre
        x = K.conv1d_tm(x, p.w, p.b, p.cout, p.k)
        n += 2
        nk = len(self.cfg["resblock_kernel_sizes"])
        for (uw, ub, ch, k, u), blocks in zip(self.ups, self.stages):
            x = K.conv_transpose1d_tm(x, uw, ub, ch, k, u, (k - u) // 2, in_slope=LRELU_SLOPE)
            n += 1
            xs = torch.empty_like(x)
            for j, block in enumerate(blocks):
                h = x
                for m, (c1, c2) in enumerate(block):
                    t = K.conv1d_tm(h, c1.w, c1.b, ch, c1.k, c1.dil, in_slope=LRELU_SLOPE, out_slope=LRELU_SLOPE)
                    if m + 1 < len(block):
                        h = K.conv1d_tm(t, c2.w, c2.b, ch, c2.k, res=h)
                    else:      # the block's last conv adds its result / nk into the stage output
                        K.conv1d_tm(t, c2.w, c2.b, ch, c2.k, res=h, out=xs, scale=1.0 / nk,
                                    acc=_lib.VOC_ACC_SET if j == 0 else _lib.VOC_ACC_ADD)
                    n += 2
            x = xs
        y = K.conv_post_tanh(x, self.post_w, self.post_b, self.post_pad, POST_SLOPE)
        self.launches = n + 1
        return y

    def synthesize_many(self, list_of_codes, dur_prediction=False):
        return [self.synthesize(c, dur_prediction=dur_prediction) for c in list_of_codes]


def vocoder_from_data_config(data_cfg, root="", device="cuda"):
    """fairseq S2SDataConfig.vocoder ({type: code_hifigan, checkpoint, config}) -> CodeHiFiGAN, or
    None when the data config has no such mapping."""
    v = (data_cfg or {}).get("vocoder")
    if not v:
        return None
    if v.get("type", "code_hifigan") != "code_hifigan":
        raise NotImplementedError(f"vocoder type '{v.get('type')}' is not supported (code_hifigan only)")
    for key in ("checkpoint", "config"):
        if not v.get(key):
            raise ValueError(f"data config vocoder: '{key}' is missing")
    path = lambda p: p if os.path.isabs(p) or not root else os.path.join(root, p)
    return CodeHiFiGAN.from_files(path(v["checkpoint"]), path(v["config"]), device)
