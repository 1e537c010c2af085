"""Isolated timing of the noise-augmentation launches (mms2ut_noise_mix_f32: partial sums, mix,
normalise) at the benchmark's batch shape: 80 utterances of clip(N(400, 120), 150, 1000) fbank
frames (~5 M samples), noise_prob 1, HIP events.  Compared with the same front end (fbank + CMVN)
with noise off, with a launch-bound floor (the same 80 utterances cut to 400 samples) and with the
algorithmic bytes (three fp32 reads and two fp32 writes of the waveform, three int16 reads of the
noise per mixed clip) at the 6.3 TB/s copy bandwidth.  Each figure: 5 warm-up calls, then 9 repeats
of 20 calls; median [min .. max] of the repeats."""
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mm = importlib.import_module("multimodal-s2ut_amd")
K, FE = mm.kernels, mm.frontend
COPY_BW = 6.3e12


def timed(fn, warm=5, reps=9, calls=20):
    for _ in range(warm):
        fn()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / calls * 1e3)
    us = np.sort(us)
    return float(np.median(us)), float(us[0]), float(us[-1])


def show(name, t, extra=""):
    print(f"{name:<44s} {t[0]:8.1f} us  [{t[1]:.1f} .. {t[2]:.1f}] {extra}", flush=True)


def main():
    rng = np.random.default_rng(0)
    fe = FE.FbankFrontend("cuda")
    frames = np.sort(np.clip(rng.normal(400, 120, 80), 150, 1000).astype(int))[::-1]
    waves = [rng.integers(-3000, 3000, 160 * int(t) + 240).astype(np.float32) for t in frames]
    clips = [rng.integers(-3000, 3000, L).astype(np.int16) for L in (48000, 160000, 90001, 16000)]
    with tempfile.TemporaryDirectory() as d:                    # NoiseAugment reads its clips from WAV files
        paths = [os.path.join(d, f"{i}.wav") for i in range(len(clips))]
        for path, c in zip(paths, clips):
            mm.manifest.write_wav(path, c)
        augs = {k: FE.NoiseAugment(paths, 1.0, [0, 20], k) for k in (1, 3)}
    samples = sum(len(w) for w in waves)
    print(f"batch: {len(waves)} utterances, {int(frames.sum())} frames, {samples} samples "
          f"({4 * samples / 1e6:.1f} MB fp32)", flush=True)

    wb = fe.upload(waves)
    show("front end, noise off (fbank + cmvn_collate)", timed(lambda: fe(wb)))

    for n_mix in (1, 3):
        aug = augs[n_mix]
        bank, boff = aug.device_bank("cuda")
        for tag, ws in (("", waves), (" (400-sample utterances: launch floor)", [w[:400] for w in waves])):
            b = fe.upload(ws)
            n = [len(w) for w in ws]
            p = aug.draws(n, np.random.RandomState(1))
            aug.check(p, n)
            params = torch.from_numpy(p).cuda()
            t = timed(lambda: K.noise_mix(b, bank, boff, params, n_mix))
            by = sum(n) * (3 * 4 + 2 * 4 + 3 * 2 * n_mix)
            show(f"noise_mix K={n_mix}{tag}"[:44], t,
                 f"{by / 1e6:6.1f} MB -> {by / t[0] / 1e3:6.0f} GB/s; at 6.3 TB/s: {by / COPY_BW * 1e6:.1f} us")

    # the loader's path: draws + validation + params upload + the three launches, then the front end
    fn = FE.FbankFrontend("cuda", noise=augs[1])
    r = np.random.RandomState(2)
    show("front end, noise on K=1 (host draws included)", timed(lambda: fn(wb, r)))
    show("front end, noise off, again", timed(lambda: fe(wb)))


if __name__ == "__main__":
    main()
