"""A numpy restatement of the noise augmentation's semantics (the reference's select_noise +
add_noise_v2 as include/mms2ut.h mms2ut_noise_mix_f32 states them) for the tests: the two sums in
fp64 (exact for 16-bit samples) rounded to fp32, then one fp32 rounding per operation.  numpy
scalar and array arithmetic on float32 never fuses a multiply with an add."""
import numpy as np

from conftest import golden_files

F32 = np.float32


def noise_signal(clips, ids):
    """int16 clips, chosen ids -> fp32 noise in [-1, 1): the clip itself, or for several clips cut
    to the shortest the floor of their mean (-1 where the integer sum is negative, else 0: Q9)."""
    if len(ids) == 1:
        return clips[int(ids[0])].astype(F32) / F32(32768.0)
    L = min(len(clips[int(i)]) for i in ids)
    s = np.sum([clips[int(i)][:L].astype(np.int64) for i in ids], axis=0)
    return np.where(s < 0, F32(-1.0), F32(0.0)).astype(F32)


def tiled_length(T, L):
    return -(-T // L) * L if T > L else L


def mix_normalised(x, noise, start, f):
    """x fp32 [T] in [-1, 1), noise fp32 [L], crop start, fp32 factor f -> fp32 [T] in [-1, 1]."""
    x, f = np.asarray(x, dtype=F32), F32(f)
    T, L = len(x), len(noise)
    assert 0 <= start and start + T <= tiled_length(T, L)
    seg = noise[(int(start) + np.arange(T, dtype=np.int64)) % L]
    clean_amp = F32(np.abs(x).sum(dtype=np.float64)) / F32(T)
    noise_amp = F32(np.abs(seg).sum(dtype=np.float64)) / F32(T)
    new_amp = f * clean_amp
    g = new_amp / (noise_amp + F32(1e-14))
    keep = F32(1.0) - f
    y = x * keep + seg * g
    assert y.dtype == F32 and type(g) is F32 and type(keep) is F32
    m = max(F32(np.abs(y).max()), F32(1.0))
    return (y / m).astype(F32)


def mix_waves(waves, clips, params):
    """The kernel's contract on a batch: ``waves`` fp32 arrays scaled by 2^15, ``params`` int32
    [B, 3 + K] rows {apply, start, bits of f, clip ids} -> new list (apply 0: the input itself)."""
    out = []
    for w, p in zip(waves, np.asarray(params)):
        if p[0] == 0:
            out.append(np.asarray(w, dtype=F32))
            continue
        f = np.array([p[2]], dtype=np.int32).view(F32)[0]
        y = mix_normalised(np.asarray(w, dtype=F32) * F32(2.0 ** -15), noise_signal(clips, p[3:]), int(p[1]), f)
        out.append(y * F32(32768.0))
    return out


def golden_cases():
    """[(name, dict)] of tests/golden/noise_*.npz (scripts/gen_noise_golden.py), loaded once."""
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = []
        for path in golden_files("noise_"):
            z = np.load(path)
            g = {k: z[k] for k in z.files}
            g["clips"] = [g[f"clip{i}"] for i in range(sum(k.startswith("clip") for k in z.files))]
            _GOLDEN.append((path.rsplit("noise_", 1)[1][:-4], g))
    return _GOLDEN


_GOLDEN = None


def golden_params(g):
    """The params row that replays a golden case's draws."""
    return np.array([[1, int(g["start"]), int(np.asarray(g["f"], dtype=F32).view(np.int32)),
                      *[int(i) for i in g["ids"]]]], dtype=np.int32)


def golden_tol(g):
    """4 d + 1 ulp of the output's peak: d is the reference's own fp32 distance from the exact
    result; the factor 4 covers this restatement's (or the kernel's) fp32 roundings on top."""
    return 4.0 * float(g["d"]) + float(np.spacing(F32(np.abs(g["out"]).max())))
