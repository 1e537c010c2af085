"""GPU fbank front end: waveforms resident in HBM -> 80-bin Kaldi log-mel -> utterance CMVN ->
zero-padded fp16 [B, Tmax, 80] (the model's src_tokens).

Moves the reference's per-utterance CPU feature extraction (speech_to_speech_dataset.py:234-274 ->
audio_utils.py:326-349 -> torchaudio.compliance.kaldi.fbank, then the data-config
utterance_cmvn transform and _collate_frames) onto the GPU: one launch for all frames of a batch,
one for CMVN + collation.  With ``--noise-config-yaml`` the reference's noise augmentation
(speech_to_speech_dataset.py:217-240) is mixed into the waveform batch first (NoiseAugment).
"""
import math

import numpy as np
import torch

from . import kernels as K

WIN, SHIFT, NFFT = 400, 160, 512


def mel_banks(num_bins=80, padded=NFFT, sample_freq=16000.0, low_freq=20.0, high_freq=0.0):
    """Triangular mel filters exactly as torchaudio.compliance.kaldi.get_mel_banks (vtln off),
    fp32, padded with a zero Nyquist column -> [num_bins, padded//2 + 1]."""
    nyq = 0.5 * sample_freq
    if high_freq <= 0.0:
        high_freq += nyq
    width = sample_freq / padded
    mlo = 1127.0 * math.log(1.0 + low_freq / 700.0)
    mhi = 1127.0 * math.log(1.0 + high_freq / 700.0)
    delta = (mhi - mlo) / (num_bins + 1)
    b = np.arange(num_bins, dtype=np.float32)[:, None]
    left = np.float32(mlo) + b * np.float32(delta)
    center = np.float32(mlo) + (b + 1.0) * np.float32(delta)
    right = np.float32(mlo) + (b + 2.0) * np.float32(delta)
    f = np.float32(width) * np.arange(padded // 2, dtype=np.float32)
    mel = (np.float32(1127.0) * np.log1p(f / np.float32(700.0)).astype(np.float32))[None, :]
    up = (mel - left) / (center - left)
    down = (right - mel) / (right - center)
    banks = np.maximum(np.float32(0.0), np.minimum(up, down)).astype(np.float32)
    return np.pad(banks, ((0, 0), (0, 1)))


def n_frames(n_samples):
    return 0 if n_samples < WIN else 1 + (n_samples - WIN) // SHIFT


class SpecAugment:
    """fairseq ``SpecAugmentTransform`` (data/audio/feature_transforms/specaugment.py) parameters
    and its per-utterance mask draws; the masking itself runs on the GPU
    (``mms2ut_specaugment_f16``).  Draw order per utterance is the transform's: freq_mask_N ×
    (f ~ U[0, F), f0 ~ U[0, nbins - f)), then, if max_t = min(T_mask, floor(T·p)) >= 1,
    time_mask_N × (t ~ U[0, max_t), t0 ~ U[0, T - t)); a zero width masks nothing.  The draws use
    a seeded numpy stream per batch (the reference's global np.random in DataLoader workers is not
    replayable, so mask positions are not bit-matched to it)."""

    def __init__(self, time_warp_W=0, freq_mask_N=0, freq_mask_F=0, time_mask_N=0, time_mask_T=0,
                 time_mask_p=0.0, mask_value=None):
        if time_warp_W:
            raise NotImplementedError("SpecAugment time warping (time_warp_W > 0) is not built")
        self.fn, self.ff = int(freq_mask_N), int(freq_mask_F)
        self.tn, self.tt, self.tp = int(time_mask_N), int(time_mask_T), float(time_mask_p)
        self.mask_value = mask_value

    @classmethod
    def from_config_dict(cls, d):
        d = d or {}
        return cls(d.get("time_warp_W", 0), d.get("freq_mask_N", 0), d.get("freq_mask_F", 0),
                   d.get("time_mask_N", 0), d.get("time_mask_T", 0), d.get("time_mask_p", 0.0),
                   d.get("mask_value", None))

    def draws(self, n_frames, nbins, rng):
        """int32 [B, 2*(freq_mask_N + time_mask_N)] of (start, width) pairs."""
        out = np.zeros((len(n_frames), 2 * (self.fn + self.tn)), dtype=np.int32)
        for b, T in enumerate(n_frames):
            T = int(T)
            for k in range(self.fn):
                f = int(rng.randint(0, self.ff)) if self.ff > 0 else 0
                out[b, 2 * k: 2 * k + 2] = (int(rng.randint(0, nbins - f)), f)
            max_t = min(self.tt, math.floor(T * self.tp))
            if max_t < 1:
                continue
            for k in range(self.tn):
                t = int(rng.randint(0, max_t))
                j = 2 * (self.fn + k)
                out[b, j: j + 2] = (int(rng.randint(0, T - t)), t)
        return out


class NoiseAugment:
    """The reference's noise augmentation (``--noise-config-yaml``: tasks/speech_to_speech.py:75-91,
    data/speech_to_speech_dataset.py:217-240 -> audio_utils.py ``select_noise`` :27-42 and
    ``add_noise_v2`` :161-233): its parameters, the noise clips (read once, kept as host int16) and
    the per-utterance draws; the mixing itself runs on the GPU (``mms2ut_noise_mix_f32``) on the
    wave batch in front of the fbank kernel.  It is applied to every split, as in the reference.

    Draw order per utterance is the reference's: u ~ U[0, 1) (mixed when u < noise_prob), then
    noise_num clip ids ~ randint(0, len(noise_wav)), then SNR = rand_fp32 * (high - low) + low, then,
    when the utterance is shorter than the tiled noise, a crop start ~ randint(0, Lt - T).  With
    noise_num > 1 the clips are cut to the shortest one and the noise is floor(mean), which for
    samples in [-1, 1) is -1 or 0.  The draws use a seeded numpy stream per batch (the
    reference's global np.random and torch streams in DataLoader workers are not replayable, so the
    chosen clips, SNRs and crop starts are not bit-matched to it); the factor
    f = 1 / (10 ** (SNR / 20) + 1) is computed in torch fp32 with the reference's operations.

    Where the reference crashes or is undefined: a scalar noise_snr s means [s, s]; noise_prob > 0
    with noise_num < 1 or no noise_wav is a ValueError here (the reference fails at the first item);
    noise files must be 16-bit PCM, mono, 16 kHz like the sources (the reference checks nothing)."""

    MAX_MIX = K.NOISE_MAX_MIX

    def __init__(self, noise_wav=(), noise_prob=0.0, noise_snr=0.0, noise_num=0):
        self.noise_wav = [str(p) for p in (noise_wav or [])]
        self.noise_prob, self.noise_num = float(noise_prob), int(noise_num)
        snr = list(noise_snr) if isinstance(noise_snr, (list, tuple)) else [noise_snr, noise_snr]
        if len(snr) != 2:
            raise ValueError(f"noise_snr: a number or [low, high] expected, got {noise_snr!r}")
        self.snr_low, self.snr_high = snr
        self.clips, self.lengths = [], np.zeros(0, dtype=np.int64)
        self._dev, self.key = {}, None
        if not self.active:
            return
        if self.noise_num < 1 or not self.noise_wav:
            raise ValueError(f"noise_prob {self.noise_prob} > 0 needs noise_num >= 1 and a non-empty noise_wav "
                             f"(got noise_num {self.noise_num}, {len(self.noise_wav)} files)")
        if self.noise_num > self.MAX_MIX:
            raise NotImplementedError(f"noise_num {self.noise_num}: at most {self.MAX_MIX} clips are mixed "
                                      "(include/mms2ut.h MMS_NOISE_MAX_MIX)")
        from .manifest import read_wav_info
        for p in self.noise_wav:
            x, sr, ch = read_wav_info(p)
            if ch != 1 or sr != 16000 or len(x) == 0:
                raise ValueError(f"{p}: noise files must be non-empty mono 16 kHz 16-bit PCM ({ch} channels, {sr} Hz)")
            self.clips.append(x.astype(np.int16))
        self.lengths = np.array([len(c) for c in self.clips], dtype=np.int64)
        import hashlib
        h = hashlib.sha1(repr((self.noise_wav, self.noise_prob, self.snr_low, self.snr_high,
                               self.noise_num)).encode())
        for c in self.clips:
            h.update(c.tobytes())
        self.key = "noise-" + h.hexdigest()[:16]

    @property
    def active(self):
        return self.noise_prob > 0

    @classmethod
    def from_config_dict(cls, d):
        d = d or {}
        return cls(d.get("noise_wav", []), d.get("noise_prob", 0.0), d.get("noise_snr", 0.0), d.get("noise_num", 0))

    def factor(self, u):
        """fp32 arrays (SNR, f) with SNR = u * (high - low) + low and f = 1 / (10 ** (SNR / 20) + 1)
        for fp32 ``u`` in [0, 1): torch fp32 tensor operations, as audio_utils.py:193-195.  The
        reference's tensors hold one element, for which torch evaluates the power with the scalar
        powf; on longer tensors it uses a SIMD power that differs in the last bit for about 1 % of
        the arguments.  So the power is taken element by element (the other operations are IEEE
        exact either way and run on the whole batch)."""
        u = torch.from_numpy(np.array(u, dtype=np.float32).reshape(-1))
        snr = u * (self.snr_high - self.snr_low) + self.snr_low
        e = snr / 20
        amp = torch.cat([10 ** e[i:i + 1] for i in range(e.numel())]) if e.numel() else e
        return snr.numpy(), (1 / (amp + 1)).numpy()

    def draws(self, n_samples, rng):
        """int32 [B, 3 + noise_num] rows {apply, start, bit pattern of the fp32 factor, clip ids}
        (include/mms2ut.h mms2ut_noise_mix_f32) for utterances of ``n_samples`` samples."""
        Kn = self.noise_num
        out = np.zeros((len(n_samples), 3 + max(Kn, 0)), dtype=np.int32)
        lengths, us = self.lengths.tolist(), []
        for b, T in enumerate(n_samples):
            T = int(T)
            if not rng.random_sample() < self.noise_prob:
                continue
            ids = rng.randint(0, len(lengths), size=Kn).tolist()
            us.append(int(rng.randint(0, 1 << 24)) * 2.0 ** -24)          # torch.rand's fp32 grid
            L = min(lengths[i] for i in ids)
            Lt = -(-T // L) * L if T > L else L
            out[b, 0], out[b, 1] = 1, int(rng.randint(0, Lt - T)) if T < Lt else 0
            out[b, 3:] = ids
        if us:
            out[out[:, 0] == 1, 2] = self.factor(us)[1].view(np.int32)
        return out

    def check(self, params, n_samples):
        """The library's convention: the host validates what the kernel indexes with."""
        p = np.asarray(params)
        Kn = p.shape[1] - 3 if p.ndim == 2 else -1
        if p.dtype != np.int32 or p.ndim != 2 or p.shape[0] != len(n_samples) or not 1 <= Kn <= self.MAX_MIX:
            raise ValueError(f"noise params: int32 [{len(n_samples)}, 3 + n_mix <= {self.MAX_MIX}] expected, "
                             f"got {p.dtype} {p.shape}")
        on = p[:, 0] != 0
        if not on.any():
            return Kn
        ids, start = p[on, 3:], p[on, 1].astype(np.int64)
        if ids.min() < 0 or ids.max() >= len(self.clips):
            raise ValueError(f"noise params: clip ids outside [0, {len(self.clips)}) in rows "
                             f"{np.flatnonzero(on)[((ids < 0) | (ids >= len(self.clips))).any(1)].tolist()}")
        L, T = self.lengths[ids].min(axis=1), np.asarray(n_samples, dtype=np.int64)[on]
        Lt = np.where(T > L, -(-T // L) * L, L)
        bad = (start < 0) | (start + T > Lt)
        if bad.any():
            raise ValueError(f"noise params: start + samples exceeds the tiled noise length in rows "
                             f"{np.flatnonzero(on)[bad].tolist()} (start {start[bad].tolist()}, samples "
                             f"{T[bad].tolist()}, tiled length {Lt[bad].tolist()})")
        return Kn

    def device_bank(self, device):
        """(int16 [sum of lengths], int64 [n_clips + 1]) on ``device``, uploaded on first use."""
        dev = torch.device(device)
        if dev not in self._dev:
            off = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
            self._dev[dev] = (torch.from_numpy(np.concatenate(self.clips)).to(dev), torch.from_numpy(off).to(dev))
        return self._dev[dev]

    def mix(self, wb, params):
        """Validate ``params`` (host int32 [B, 3 + n_mix]) against the wave batch and mix in place."""
        p = np.ascontiguousarray(params)
        n_mix = self.check(p, wb["n_samples"])
        if not p[:, 0].any():
            return wb
        dev = wb["wave"].device
        bank, off = self.device_bank(dev)
        K.noise_mix(wb, bank, off, torch.from_numpy(p).pin_memory().to(dev, non_blocking=True), n_mix)
        return wb


_NOISE_BANKS = {}


def register_noise_bank(key, aug):
    """The fairseq path hands only a string key through the collater (DataLoader workers); the
    dataset registers its NoiseAugment in the main process, which runs the model's forward."""
    _NOISE_BANKS[key] = aug
    return key


def noise_bank(key):
    if key not in _NOISE_BANKS:
        raise KeyError(f"noise bank {key!r} is not registered in this process (frontend.register_noise_bank)")
    return _NOISE_BANKS[key]


_FRONTENDS = {}


def wave_net_input_src(ni, device):
    """fp16 [B, Tmax, 80] src_tokens for a sample whose net_input carries waveforms instead of
    features (the fairseq-train drop-in's collater, fairseq_adapter.py): ``src_waves`` int32 [N]
    = the fp32 samples' bit patterns (so fairseq's apply_half leaves them alone), ``src_wave_offsets``
    int64 [B + 1], ``src_cmvn`` bool, optional ``src_specaugment`` {masks int32 [B, 2(nf + nt)],
    n_freq, n_time, mask_value} drawn by the collater (CPU worker, as the reference's transform),
    optional ``src_noise`` {params int32 [B, 3 + K] (NoiseAugment.draws; the factor travels as a bit
    pattern, so apply_half leaves it alone), n_mix K, bank: a frontend.register_noise_bank key}:
    the waveforms are mixed with noise before the fbank."""
    dev = torch.device(device)
    cmvn = bool(ni.get("src_cmvn", True))
    fe = _FRONTENDS.get((dev, cmvn))
    if fe is None:
        fe = _FRONTENDS[(dev, cmvn)] = FbankFrontend(dev, cmvn=cmvn)
    w = ni["src_waves"]
    if w.dtype != torch.int32:
        raise TypeError(f"src_waves: int32 bit patterns of fp32 samples expected, got {w.dtype}")
    sn = ni.get("src_noise")
    wf = w.to(dev).view(torch.float32)
    if sn is not None and wf.data_ptr() == w.data_ptr():
        wf = wf.clone()                            # the mix is in place: leave the sample's tensor alone
    wb = fe.from_device(wf, ni["src_wave_offsets"])
    if sn is not None:
        p = sn["params"]
        if p.dtype != torch.int32 or p.dim() != 2 or p.shape[1] != 3 + int(sn["n_mix"]):
            raise TypeError(f"src_noise: int32 [B, 3 + {sn['n_mix']}] params expected, got {p.dtype} {tuple(p.shape)}")
        noise_bank(sn["bank"]).mix(wb, p.cpu().numpy())
    feats = K.fbank(wb["wave"], wb["wave_off"], wb["frame_off"], wb["total"], fe.banks, fe.mel_range, fe.num_bins)
    out = K.cmvn_collate(feats, wb["frame_off"], wb["B"], wb["Tmax"], fe.num_bins, cmvn)
    sa = ni.get("src_specaugment")
    if sa is not None and sa["n_freq"] + sa["n_time"] > 0:
        K.specaugment(out, wb["frame_off"], sa["masks"].to(dev, torch.int32).contiguous(), int(sa["n_freq"]),
                      int(sa["n_time"]), sa.get("mask_value"))
    return out


class FbankFrontend:
    def __init__(self, device="cuda", num_bins=80, cmvn=True, specaugment=None, noise=None):
        self.device = torch.device(device)
        self.num_bins = num_bins
        self.cmvn = cmvn
        self.specaugment = specaugment
        self.noise = noise if noise is not None and noise.active else None
        banks = mel_banks(num_bins)
        self.banks = torch.from_numpy(banks).to(self.device)
        nz = banks > 0
        lo = nz.argmax(1)
        hi = banks.shape[1] - nz[:, ::-1].argmax(1)
        lo[~nz.any(1)] = hi[~nz.any(1)] = 0
        rng = np.stack([lo, hi], 1).astype(np.int32)
        if int((hi - lo).sum()) > 1024:
            raise ValueError("fbank: more than 1024 nonzero mel weights (include/mms2ut.h mms2ut_fbank_f32)")
        self.mel_range = torch.from_numpy(rng.reshape(-1)).to(self.device)

    def upload(self, waves, pin=False):
        """waves: list of 1-D float32 arrays already in int16 range (get_waveform(normalization=False)).
        Returns a device-resident wave batch (sorted by frames, descending, like the collater).
        pin=True stages the samples in pinned host memory and copies asynchronously."""
        lens = [n_frames(len(w)) for w in waves]
        order = sorted(range(len(waves)), key=lambda i: -lens[i])
        waves = [waves[i] for i in order]
        fr = np.array([lens[i] for i in order], dtype=np.int64)
        wl = np.array([len(w) for w in waves], dtype=np.int64)
        wave_off = np.concatenate([[0], np.cumsum(wl)]).astype(np.int64)
        frame_off = np.concatenate([[0], np.cumsum(fr)]).astype(np.int32)
        flat = np.concatenate(waves).astype(np.float32)
        def dev(a):
            t = torch.from_numpy(a)
            return t.pin_memory().to(self.device, non_blocking=True) if pin else t.to(self.device)

        return {
            "wave": dev(flat), "wave_off": dev(wave_off), "frame_off": dev(frame_off),
            "n_frames": torch.from_numpy(fr), "total": int(fr.sum()), "Tmax": int(fr.max()),
            "B": len(waves), "order": order, "n_samples": wl,
        }

    def __call__(self, wb, rng=None):
        """-> fp16 [B, Tmax, nbins].  With a SpecAugment policy and a numpy RandomState ``rng``
        (training batches), the masks are drawn on the host and applied in place after CMVN.  With a
        NoiseAugment and an ``rng`` (every split), the noise draws come first from the same stream and
        the wave batch is mixed in place before the fbank (so a wave batch is consumed once)."""
        if self.noise is not None and rng is not None:
            self.noise.mix(wb, self.noise.draws(wb["n_samples"].tolist(), rng))
        feats = K.fbank(wb["wave"], wb["wave_off"], wb["frame_off"], wb["total"], self.banks, self.mel_range,
                        self.num_bins)
        out = K.cmvn_collate(feats, wb["frame_off"], wb["B"], wb["Tmax"], self.num_bins, self.cmvn)
        sa = self.specaugment
        if sa is not None and rng is not None and sa.fn + sa.tn > 0:
            m = sa.draws(wb["n_frames"].tolist(), self.num_bins, rng)
            masks = torch.from_numpy(m).pin_memory().to(self.device, non_blocking=True)
            K.specaugment(out, wb["frame_off"], masks, sa.fn, sa.tn, sa.mask_value)
        return out

    def from_device(self, waves, wave_off):
        """A wave batch from samples already in HBM: ``waves`` fp32 [N] (utterances back to back, in
        the collater's frame-descending order), ``wave_off`` int64 [B + 1] sample offsets."""
        off = wave_off.cpu().numpy().astype(np.int64)
        fr = np.array([n_frames(int(n)) for n in np.diff(off)], dtype=np.int64)
        if len(fr) == 0 or np.any(fr <= 0) or np.any(np.diff(fr) > 0):
            raise ValueError(f"wave batch: frames {fr.tolist()} (need >= 1 frame each, descending order)")
        frame_off = np.concatenate([[0], np.cumsum(fr)]).astype(np.int32)
        return {"wave": waves.contiguous(), "wave_off": wave_off.to(self.device, torch.int64).contiguous(),
                "frame_off": torch.from_numpy(frame_off).to(self.device), "n_frames": torch.from_numpy(fr),
                "total": int(fr.sum()), "Tmax": int(fr.max()), "B": len(fr), "order": list(range(len(fr))),
                "n_samples": np.diff(off)}

    def features_f32(self, wb):
        """Raw log-mel features [total_frames, nbins] fp32 (no CMVN) — for parity tests."""
        return K.fbank(wb["wave"], wb["wave_off"], wb["frame_off"], wb["total"], self.banks, self.mel_range,
                       self.num_bins)
