"""Golden fixtures for the noise augmentation, written by running the reference's OWN code.

Imports ``mm_s2ut/data/audio_utils.py`` from the reference under the import shim of SURVEY.md
Appendix S (fairseq stubbed; ``soundfile`` and ``wavfile`` added to the served names, the stub
``soundfile.read`` returning in-memory arrays so that ``select_noise`` runs unmodified) and calls
``select_noise`` and ``add_noise_v2(..., noise_waveform_start=-1, add_white_noise=False,
normalize=True)`` the way the dataset does (speech_to_speech_dataset.py:217-232).  Writes
``tests/golden/noise_<case>.npz``:

  clean int16 [T], clip0.. int16, ids (the clips select_noise drew), noise_num, snr_range,
  snr / start (what the reference drew, recovered by re-seeding and replaying its two torch draws),
  f (fp32 factor, same three torch operations), out (the reference's fp32 output, samples in
  [-1, 1]) and d = max|out - out64|: the reference's distance from this script's float64
  evaluation of the same formulas, the yardstick of the tests' tolerance.

This script contains no reference source and never runs on a GPU machine: it needs the reference
checkout (``MMS2UT_REFERENCE``, default ``/root/reference``) and skips itself when that is absent.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_noise_golden.py
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("MMS2UT_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")

_FILES = {}      # path -> int16 samples served by the stub soundfile.read


class _Anything:
    def __init__(self, *a, **k):
        pass


class _AutoMod(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if self.__name__ == "soundfile" and name == "read":
            # soundfile.read's default: float64 in [-1, 1), mono files as [T]
            return lambda path, *a, **k: (_FILES[path].astype(np.float64) / 32768.0, 16000)
        return type(name, (_Anything,), {})


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in ("fairseq", "soundfile", "wavfile"):
            return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        m = _AutoMod(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, m):
        pass


def _cases():
    """name -> (clean int16, [clips int16], noise_num, (snr low, high), seed, normalises or None)"""
    r = np.random.default_rng(20240)
    i16 = lambda x: np.clip(np.round(x), -32768, 32767).astype(np.int16)   # noqa: E731

    def speech(T, amp):
        t = np.arange(T)
        return i16(amp * (np.sin(0.07 * t) * np.sin(0.0031 * t + 1.0) + 0.15 * r.standard_normal(T)))

    def hiss(L, amp):
        return i16(amp * r.standard_normal(L))

    spiky = hiss(4001, 20.0)
    spiky[::250] = 32767
    spiky[125::250] = -32768
    return {
        "a": (speech(3000, 6000.0), [hiss(5000, 1500.0)], 1, (5, 15), 11, False),
        "b": (speech(2500, 12000.0), [spiky], 1, (0, 0), 12, True),
        "c": (speech(2700, 6000.0), [hiss(1000, 900.0), hiss(1300, 900.0)], 1, (0, 20), 13, None),
        "d": (speech(2000, 5000.0), [hiss(2000, 2500.0)], 1, (-5, 5), 14, None),
        "e": (speech(1500, 6000.0), [hiss(3000, 700.0), hiss(2200, 700.0), hiss(4100, 700.0), hiss(2600, 700.0)],
              3, (0, 10), 15, None),
        "f": (speech(400, 7000.0), [hiss(700, 2000.0)], 1, (10, 10), 16, None),
    }


def _out64(x, seg, f):
    """The mixing formulas in float64 (f: the fp32 factor the reference used)."""
    x, seg, f = x.astype(np.float64), seg.astype(np.float64), float(f)
    T = len(x)
    g = f * (np.abs(x).sum() / T) / (np.abs(seg).sum() / T + 1e-14)
    y = x * (1.0 - f) + seg * g
    return y / max(np.abs(y).max(), 1.0), np.abs(y).max()


def main():
    if not os.path.isdir(REF):
        print("reference absent; nothing to do")
        return 0
    sys.path.insert(0, REF)
    sys.meta_path.insert(0, _Finder())
    import mm_s2ut.data.audio_utils as AU  # noqa: E402  (reference code, shimmed deps)

    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, (clean, clips, num, (lo, hi), seed, normalises) in _cases().items():
        paths = [f"mem://{name}/{i}.wav" for i in range(len(clips))]
        _FILES.update(zip(paths, clips))
        np.random.seed(seed)
        torch.manual_seed(seed)
        noise = AU.select_noise(paths, num)                              # [L, 1] float32
        x = torch.from_numpy((clean.astype(np.float32) / np.float32(32768.0))[None, :].copy())
        nz = torch.from_numpy(np.ascontiguousarray(noise.transpose()))
        noise_sig = nz[0].numpy().copy()                                 # before the in-place scaling
        out = AU.add_noise_v2(waveforms=x, noise_waveform=nz, snr_low=lo, snr_high=hi, noise_waveform_start=-1,
                              add_white_noise=False, normalize=True)[0].numpy()
        # replay the draws: ids from numpy, then the two torch draws in the reference's order
        np.random.seed(seed)
        ids = np.random.randint(0, len(paths), size=num)
        torch.manual_seed(seed)
        snr = torch.rand(1, 1) * (hi - lo) + lo
        f = (1 / (10 ** (snr / 20) + 1)).numpy().reshape(())
        T, L = len(clean), len(noise_sig)
        assert L == min(len(clips[i]) for i in ids)
        Lt = -(-T // L) * L if T > L else L
        start = int(torch.randint(0, Lt - T, size=(1,)).item()) if T < Lt else 0
        seg = noise_sig[(start + np.arange(T)) % L]
        o64, peak = _out64(x[0].numpy(), seg, f)
        d = float(np.abs(out.astype(np.float64) - o64).max())
        assert d < 1e-5, f"case {name}: the replayed draws do not reproduce the reference's output (d = {d})"
        if normalises is not None:
            assert (peak > 1.0) == normalises, f"case {name}: max|y| = {peak}, normalisation expected {normalises}"
        path = os.path.join(OUT, f"noise_{name}.npz")
        np.savez_compressed(path, clean=clean, ids=ids.astype(np.int64), noise_num=np.int64(num),
                            snr_range=np.array([lo, hi], dtype=np.float64), snr=snr.numpy().reshape(()),
                            start=np.int64(start), f=f.astype(np.float32), out=out.astype(np.float32),
                            d=np.float64(d), peak=np.float64(peak),
                            **{f"clip{i}": c for i, c in enumerate(clips)})
        total += os.path.getsize(path)
        print(f"noise_{name}: T={T} L={L} ids={ids.tolist()} snr={float(snr):.4f} start={start} f={float(f):.6f} "
              f"max|y|={peak:.4f} d={d:.3e} ({os.path.getsize(path)} B)")
    assert total < 300 * 1024, f"fixtures too large: {total} B"
    return 0


if __name__ == "__main__":
    sys.exit(main())
