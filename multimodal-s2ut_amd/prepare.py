"""S2UT data preparation, the reference's ``scripts/preprocess/`` stage around the unit quantiser:

  * ``1_preprocess.ipynb`` (``ffmpeg -ar 16000``)                 -> ``Resampler`` / ``convert_dir``
  * ``2_manifest.sh`` (fairseq ``wav2vec_manifest.py``)           -> ``write_manifest``
  * ``3_cluster.sh``                                              -> units.quantize_manifest (built before)
  * ``5_prep_s2ut_data.sh`` (fairseq ``prep_s2ut_data.py``)       -> ``prep_s2ut_data``

The rate conversion is the device part (``csrc/resample.hip``): bandlimited sinc interpolation in the
polyphase form of ``torchaudio.functional.resample``, restated from its published source.  For
``orig -> new`` Hz with g = gcd, o = orig / g, n = new / g:

    base = min(o, n) rolloff;  width = ceil(lpw o / base);  K = 2 width + o taps per phase
    t = clamp((-i / n + (c - width) / o) base, -lpw, lpw)            phase i < n, tap c < K
    h[i][c] = sinc(pi t) w(t) base / o
    w(t) = I0(beta sqrt(1 - (t / lpw)^2)) / I0(beta)   (kaiser)   or   cos^2(pi t / (2 lpw))   (hann)
    y[j n + i] = sum_c h[i][c] xp[j o + c],   xp[t] = x[t - width] inside the clip, 0 outside

and a clip of L samples gives ceil(n L / o) samples.  The defaults are torchaudio's "kaiser_best" set.
The taps are computed here in float64 and rounded to fp32 once.  torchaudio, sox and ffmpeg are not
build dependencies, so the filter is not pinned against any of them, and it is not bit-equal to ffmpeg's
swresample (a different filter design); it is checked against a float64 restatement of the formulas
above (tests/resample_ref.py).

Everything else here is host code that has to agree with the loaders already in the tree:
``units.read_manifest`` reads what ``write_manifest`` writes, and ``manifest.MultiModalS2SManifest`` loads
what ``prep_s2ut_data`` writes.  Compressed audio (mp3) and sample formats other than 16-bit PCM are
refused by name; decoding them stays outside.
"""
import concurrent.futures as cf
import itertools
import math
import os
import re
import shutil
import wave

import numpy as np

from . import manifest as M

LOWPASS_FILTER_WIDTH = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
MAX_TAPS = 1 << 20          # kernels.RESAMPLE_MAX_TAPS: a 4 MiB table, one XCD's L2


def resample_taps(orig, new, lowpass_filter_width=LOWPASS_FILTER_WIDTH, rolloff=ROLLOFF, window="kaiser", beta=BETA):
    """-> (h fp32 [n, K], width, o, n) for ``orig -> new`` Hz (module docstring).  Refuses rate pairs whose
    table n K would exceed MAX_TAPS (e.g. 44101 -> 16000: o = 44101, n = 16000)."""
    orig, new = int(orig), int(new)
    if orig < 1 or new < 1:
        raise ValueError(f"resample: sample rates must be positive (got {orig} -> {new})")
    if lowpass_filter_width < 1 or not 0.0 < rolloff <= 1.0:
        raise ValueError(f"resample: lowpass_filter_width {lowpass_filter_width} >= 1 and 0 < rolloff {rolloff} <= 1")
    if window not in ("kaiser", "hann"):
        raise ValueError(f"resample: window '{window}' (kaiser or hann)")
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    lpw = float(lowpass_filter_width)
    width = math.ceil(lpw * o / base)
    K = 2 * width + o
    if n * K > MAX_TAPS:
        raise ValueError(f"resample {orig} -> {new} Hz: {n} phases x {K} taps = {n * K} taps exceed the cap of "
                         f"{MAX_TAPS} (the rates share too small a divisor; convert through a common rate)")
    c = np.arange(K, dtype=np.float64)[None, :]
    i = np.arange(n, dtype=np.float64)[:, None]
    t = np.clip((-i / n + (c - width) / o) * base, -lpw, lpw)
    if window == "hann":
        w = np.cos(t * math.pi / lpw / 2) ** 2
    else:
        w = np.i0(beta * np.sqrt(1 - (t / lpw) ** 2)) / np.i0(beta)
    h = np.sinc(t) * w * (base / o)          # np.sinc(t) = sin(pi t) / (pi t), 1 at 0
    return h.astype(np.float32), width, o, n


def out_len(n_samples, o, n):
    return (int(n_samples) * n + o - 1) // o


class Resampler:
    """``orig -> new`` Hz on ``device``: the tap table is built once and kept tap-major in HBM."""

    def __init__(self, orig, new, lowpass_filter_width=LOWPASS_FILTER_WIDTH, rolloff=ROLLOFF, window="kaiser",
                 beta=BETA, device="cuda"):
        import torch
        self.orig, self.new = int(orig), int(new)
        self.device = torch.device(device)
        self.h, self.width, self.o, self.n = resample_taps(orig, new, lowpass_filter_width, rolloff, window, beta)
        self.K = self.h.shape[1]
        self.identity = self.o == self.n
        self.taps = None
        if not self.identity:
            from . import kernels
            kernels.resample_tile(self.o, self.n, self.K)     # the kernel's own limits, at construction
            self.taps = torch.from_numpy(np.ascontiguousarray(self.h.T)).to(self.device)

    def _run(self, clips, int16):
        import torch
        clips = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in clips]
        for k, c in enumerate(clips):
            if c.size == 0:
                raise ValueError(f"resample: clip {k} is empty")
        if not clips:
            return [], []
        off = np.concatenate([[0], np.cumsum([c.size for c in clips])]).astype(np.int64)
        x = torch.from_numpy(np.concatenate(clips)).to(self.device)
        if self.identity:                    # orig == new: the input's bits
            y, out_off = x, off
            y16 = x.round().clamp_(-32768, 32767).to(torch.int16) if int16 else None
        else:
            from . import kernels
            y, out_off, y16 = kernels.resample(x, off, self.taps, self.o, self.n, self.width, int16=int16)
        cut = lambda t: [t[out_off[b]:out_off[b + 1]] for b in range(len(clips))]
        return cut(y), (cut(y16) if int16 else [])

    def __call__(self, clips):
        """list of fp32 arrays (mono, any scale) -> list of fp32 device tensors, in order."""
        return self._run(clips, False)[0]

    def to_int16(self, clips):
        """list of fp32 arrays in int16 range -> list of int16 device tensors: rint, then clip to
        [-32768, 32767] (``manifest.write_wav``'s rounding), written by the same launch."""
        return self._run(clips, True)[1]


def _wav_files(root, ext=".wav"):
    ext = ext if ext.startswith(".") else "." + ext
    found = []
    for d, _, files in os.walk(root):
        found += [os.path.relpath(os.path.join(d, f), root) for f in files if f.endswith(ext)]
    return sorted(found)


def wav_header(path):
    """(sample rate, channels, sample width in bytes, frames) of a PCM WAV, from its header; compressed
    or non-PCM files are a ValueError that names the file."""
    try:
        with wave.open(path, "rb") as w:
            return w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
    except (wave.Error, EOFError) as e:
        raise ValueError(f"{path}: not a PCM WAV file ({e}); decode compressed audio to 16-bit PCM first") from None


def convert_dir(src_dir, dst_dir, rate=16000, batch_size=64, num_workers=8, device="cuda", progress=None):
    """Every ``*.wav`` under src_dir, recursively -> 16-bit mono ``rate`` Hz at the same relative path under
    dst_dir.  Reading (manifest.read_wav_info: 16-bit PCM, channels averaged) and writing run on a pool of
    num_workers threads while the device resamples the previous batch; clips are grouped by source rate
    (one tap table per rate).  Files already mono at ``rate`` are copied sample for sample, and a tree of
    only such files needs no GPU.  -> {"files", "copied", "resampled": {rate: count}}."""
    if batch_size < 1 or num_workers < 1:
        raise ValueError("batch_size and num_workers must be >= 1")
    files = _wav_files(src_dir)
    if not files:
        raise ValueError(f"{src_dir}: no .wav files")
    groups, copies = {}, []
    for rel in files:
        path = os.path.join(src_dir, rel)
        sr, ch, sw, _ = wav_header(path)
        if sw != 2:
            raise ValueError(f"{path}: only 16-bit PCM WAV is supported (got {8 * sw}-bit)")
        if sr == rate and ch == 1:
            copies.append(rel)
        else:
            groups.setdefault(sr, []).append(rel)
    for rel in files:
        os.makedirs(os.path.dirname(os.path.join(dst_dir, rel)) or ".", exist_ok=True)
    done = 0

    def read(rel):
        x = M.read_wav_info(os.path.join(src_dir, rel))[0]
        if x.size == 0:
            raise ValueError(f"{os.path.join(src_dir, rel)}: no samples")
        return x

    def copy(rel):
        shutil.copyfile(os.path.join(src_dir, rel), os.path.join(dst_dir, rel))

    with cf.ThreadPoolExecutor(max_workers=num_workers) as pool:
        for _ in pool.map(copy, copies):
            done += 1
            if progress:
                progress(done, len(files))
        writes = []
        for sr in sorted(groups):
            rs = Resampler(sr, rate, device=device)
            rels = groups[sr]
            batches = [rels[i:i + batch_size] for i in range(0, len(rels), batch_size)]
            pending = [pool.submit(read, r) for r in batches[0]]
            for i, batch in enumerate(batches):
                clips = [f.result() for f in pending]
                pending = [pool.submit(read, r) for r in batches[i + 1]] if i + 1 < len(batches) else []
                outs = [t.cpu().numpy() for t in rs.to_int16(clips)]
                for f in writes:                 # the batch before this one: at most two batches are held
                    f.result()
                writes = [pool.submit(M.write_wav, os.path.join(dst_dir, r), s, rate) for r, s in zip(batch, outs)]
                done += len(batch)
                if progress:
                    progress(done, len(files))
        for f in writes:
            f.result()
    return {"files": len(files), "copied": len(copies), "resampled": {sr: len(v) for sr, v in groups.items()}}


def write_manifest(root, dest_tsv, ext=".wav"):
    """fairseq ``examples/wav2vec/wav2vec_manifest.py --valid-percent 0``: the absolute root on line 1, then
    ``relative/path<TAB>n_samples`` per file found under it (recursively), sample counts from the headers,
    in sorted order.  ``units.read_manifest`` reads it back.  -> the number of files."""
    root = os.path.realpath(root)
    if not os.path.isdir(root):
        raise FileNotFoundError(f"{root}: not a directory")
    files = _wav_files(root, ext)
    if not files:
        raise ValueError(f"{root}: no files ending in '{ext}'")
    lines = [root]
    for rel in files:
        if "\t" in rel or "\n" in rel:
            raise ValueError(f"{os.path.join(root, rel)}: tab or newline in a file name")
        lines.append(f"{rel}\t{wav_header(os.path.join(root, rel))[3]}")
    os.makedirs(os.path.dirname(os.path.abspath(dest_tsv)), exist_ok=True)
    with open(dest_tsv, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(files)


def load_units(path):
    """The quantiser's output (units.quantize_manifest): one ``id|u u u`` line per file -> {id: units string}."""
    out = {}
    with open(path) as f:
        for k, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if not line.strip():
                continue
            sid, sep, units = line.partition("|")
            if not sep:
                raise ValueError(f"{path}:{k}: 'id|units' expected, got {line!r}")
            out[sid] = units.strip()
    return out


def process_units(units, reduce=False):
    """prep_s2ut_data's ``process_units``: the unit strings, with runs of equal units merged when reduce."""
    u = units.split()
    return [k for k, _ in itertools.groupby(u)] if reduce else u


def _natural(stem):
    return [(0, int(p), "") if p.isdigit() else (1, 0, p) for p in re.split(r"(\d+)", stem) if p]


MANIFEST_COLUMNS = ["id", "src_audio", "src_n_frames", "tgt_text", "tgt_n_frames"]
# fairseq S2TDataConfigWriter.set_specaugment_lb_policy: LibriSpeech basic, no time warp
SPECAUGMENT_LB = {"time_warp_W": 0, "freq_mask_N": 1, "freq_mask_F": 27, "time_mask_N": 1,
                  "time_mask_T": 100, "time_mask_p": 1.0}


def write_config_yaml(output_root, vocoder_checkpoint, vocoder_cfg):
    """prep_s2ut_data's ``gen_config_yaml(specaugment_policy="lb", feature_transform=["utterance_cmvn"],
    vocoder_type="code_hifigan")``, with the key names frontend.SpecAugment.from_config_dict reads (fairseq's
    writer spells the warp key ``time_wrap_W``; it is 0 either way)."""
    import yaml
    cfg = {
        "input_channels": 1,
        "input_feat_per_channel": 80,
        "specaugment": dict(SPECAUGMENT_LB),
        "transforms": {"*": ["utterance_cmvn"], "_train": ["utterance_cmvn", "specaugment"]},
    }
    if vocoder_cfg or vocoder_checkpoint:      # called without either (from Python): no vocoder entry
        cfg["vocoder"] = {"type": "code_hifigan", "config": os.fspath(vocoder_cfg),
                          "checkpoint": os.fspath(vocoder_checkpoint)}
    path = os.path.join(output_root, "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f, default_flow_style=False, sort_keys=True)
    return path


def prep_s2ut_data(source_dir, target_dir, splits, output_root, reduce_unit=False, vocoder_checkpoint="",
                   vocoder_cfg=""):
    """fairseq ``examples/speech_to_speech/preprocessing/prep_s2ut_data.py`` as the reference calls it
    (5_prep_s2ut_data.sh).  Per split: units from ``{target_dir}/{split}.txt``, sources
    ``{source_dir}/{split}/*.wav`` in natural numeric order of the stems -> ``{output_root}/{split}.tsv``
    (id = stem, src_audio = absolute path, src_n_frames = samples // 160, tgt_text = units, tgt_n_frames =
    unit count); then ``config.yaml``.  The unit column is ``tgt_text``, the name the reference's dataset
    and manifest.py read (stock fairseq writes ``tgt_audio``).  Sources without units are skipped.
    Multi-channel 16 kHz sources pass, as in fairseq (manifest.read_wav averages the channels); with both
    vocoder paths empty config.yaml gets no ``vocoder`` entry.
    -> {split: {"written": count, "missing": [ids]}}."""
    if isinstance(splits, str):
        splits = [splits]
    os.makedirs(output_root, exist_ok=True)
    report = {}
    for split in splits:
        units = load_units(os.path.join(target_dir, f"{split}.txt"))
        src = os.path.join(source_dir, split)
        if not os.path.isdir(src):
            raise FileNotFoundError(f"{src}: no source directory for split '{split}'")
        stems = sorted((f[:-4] for f in os.listdir(src) if f.endswith(".wav")), key=_natural)
        rows, missing = [], []
        for stem in stems:
            if stem not in units:
                missing.append(stem)
                continue
            path = os.path.abspath(os.path.join(src, stem + ".wav"))
            sr, _, sw, frames = wav_header(path)       # any channel count: the loader folds to mono, as fairseq's
            if sr != 16000:
                raise ValueError(f"{path}: {sr} Hz; the S2UT sources are 16 kHz "
                                 "(convert the corpus with scripts/mms2ut_resample.py first)")
            if sw != 2:
                raise ValueError(f"{path}: only 16-bit PCM WAV is supported (got {8 * sw}-bit)")
            u = process_units(units[stem], reduce_unit)
            if not u:
                raise ValueError(f"{os.path.join(target_dir, split + '.txt')}: no units for '{stem}'")
            if "\t" in path:
                raise ValueError(f"{path}: tab in a file name")
            rows.append([stem, path, str(frames // 160), " ".join(u), str(len(u))])
        if not rows:
            raise ValueError(f"{src}: no source with units in {os.path.join(target_dir, split + '.txt')}")
        with open(os.path.join(output_root, f"{split}.tsv"), "w") as f:
            f.write("\n".join("\t".join(r) for r in [MANIFEST_COLUMNS] + rows) + "\n")
        report[split] = {"written": len(rows), "missing": missing}
    write_config_yaml(output_root, vocoder_checkpoint, vocoder_cfg)
    return report


def report_lines(report):
    """prep_s2ut_data's closing messages, one per split."""
    out = []
    for split, r in report.items():
        line = f"{split}: processed {r['written']} samples"
        if r["missing"]:
            line += (f"; {len(r['missing'])} with missing target data "
                     f"(first 3 examples: {', '.join(r['missing'][:3])})")
        out.append(line)
    return out
