"""GPU: the wav2vec2 CTC kernels (csrc/asr.hip) and the Wav2Vec2CTC forward built on them, against the
fp32 CPU restatement in tests/asr_ref.py.

Tolerances are measured, not chosen (the convention of tests/test_gpu_vocoder.py): a GPU result may be at
most TOL_FACTOR (3) x as far from the fp32 restatement (max-abs) as the restatement's own fp16-storage
emulation is for the same inputs -- the GPU rounds at the same places as the emulation, only the fp32
summation order differs.  Every check prints its floor and ratio.  Argmax ids are compared on the frames
whose fp32 top-2 margin is at least 2 x allowance (both sides are then within allowance of the same
logits, so the order of the top two cannot flip); tests/test_asr.py bounds the share of other frames.

asr_conv's block owns 128 output positions, or 32 where its waves split the reduction (at least 4 K-steps
and fewer than 256 blocks of 128, the vocoder's rule), and 64 output channels; the input channels pass
through LDS in slices of 64.  Short utterances and the small config only ever reach the 32-position
kernel, so the kernel tests name the variant each shape takes (conv_dispatch.splits restates the rule) and
hold shapes on both sides of it: at the real width the 128-position kernel runs layer 1 from about 2.6 s of
audio."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import asr_ref as AR
from conftest import ROOT, pkg
from conv_dispatch import splits as _splits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def A():
    return pkg("asr")


@pytest.fixture(scope="module")
def V():
    return pkg("vocoder")


@pytest.fixture(scope="module")
def K():
    return pkg("kernels")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _check(name, got, ref, emu):
    """got within TOL_FACTOR x the emulation's distance from the fp32 restatement -> the allowance."""
    floor = float((emu - ref).abs().max())
    err = float((got.float().cpu() - ref).abs().max())
    print(f"{name}: emulation floor {floor:.3e}, GPU error {err:.3e} ({err / floor if floor else float('nan'):.2f}x)")
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()
    assert floor > 0 and err <= AR.TOL_FACTOR * floor, (name, err, floor)
    return AR.TOL_FACTOR * floor


_MODELS = {}


def _model(A, cfg_name, seed, blank_bias=0.0):
    key = (cfg_name, seed, blank_bias)
    if key not in _MODELS:
        cfg = {"small": AR.SMALL, "wide": AR.WIDE}[cfg_name]
        _MODELS[key] = A.Wav2Vec2CTC(AR.make_state_dict(cfg, seed, blank_bias=blank_bias), cfg, AR.VOCAB, device=DEV)
    return _MODELS[key]


# ------------------------------------------------------------------------------------------ kernels

@pytest.mark.parametrize("T,Cin,Cout,k,s,split", [
    (37, 64, 64, 3, 2, True),        # odd T: the trailing row is unused
    (130, 64, 72, 2, 2, True),       # Cout off the 64-grid: a second, narrow channel block
    (261, 128, 64, 3, 2, True),      # two Cin slices; 130 outputs: a ragged last 32-position block
    (70, 512, 512, 3, 2, True),      # the real width
    # the 128-position kernel (every wave walks all K-steps, 257 staged rows per block):
    (300, 32, 72, 3, 2, False),      # 3 K-steps; 149 outputs: a ragged second block; Cout off the 64-grid
    (257, 32, 64, 2, 2, False),      # 2 K-steps, exactly one full block of 128 outputs
    (8195, 512, 512, 3, 2, False)])  # the real width at 2.6 s of audio: 33 x 8 = 264 blocks, one output in the last
def test_strided_conv_with_ln_gelu_tail(V, K, T, Cin, Cout, k, s, split):
    assert _splits((T - k) // s + 1, Cin, Cout, k) == split
    g = _gen(T + Cin)
    x, W, b = torch.randn(T, Cin, generator=g), torch.randn(Cout, Cin, k, generator=g) / (Cin * k) ** 0.5, \
        0.1 * torch.randn(Cout, generator=g)
    lg, lb = 1.0 + 0.1 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
    ref_c, emu_c = AR.conv_strided(x, W, b, s), AR.conv_strided(x, W, b, s, emulate=True)
    got = K.asr_conv(x.half().to(DEV), V.pack_conv_weight(W).to(DEV), b.to(DEV), Cout, k, s)
    assert got.shape[0] == (T - k) // s + 1
    _check(f"asr_conv {Cin}->{Cout} k{k} s{s} T{T}", got, ref_c, emu_c)
    K.asr_ln_gelu(got, lg.to(DEV), lb.to(DEV))
    _check(f"  + LN + GELU", got, AR.ln_gelu(ref_c, lg, lb), AR.ln_gelu(emu_c, lg, lb, emulate=True))


@pytest.mark.parametrize("n,dc", [(400, 0.0), (719, 0.0), (8000, 0.4)])
def test_layer0_and_statistics(K, n, dc):
    """One frame, one frame with unused trailing samples, many blocks; the last with a DC offset far above
    the signal's standard deviation (the variance is a mean squared deviation, not E[x^2] - mean^2)."""
    g = _gen(n)
    x = AR.to_float(AR.make_wave(n, n, dc=dc))
    C, k, s = 64, 10, 5
    W, b = torch.randn(C, 1, k, generator=g) / k ** 0.5, 0.1 * torch.randn(C, generator=g)
    lg, lb = 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    xd = x.to(DEV)
    stats = K.wave_stats(xd, AR.NORM_EPS).cpu().double()
    x64 = x.double()
    want = torch.stack([x64.mean(), 1.0 / torch.sqrt(x64.var(unbiased=False) + AR.NORM_EPS)])
    rel = float(((stats - want).abs() / want.abs().clamp_min(1e-3)).max())
    print(f"wave_stats n{n} dc{dc}: mean {float(stats[0]):.6f}, rstd {float(stats[1]):.4f}, rel err {rel:.2e}")
    assert rel <= 2.0 ** -22          # double accumulation, one rounding to fp32 (2^-24) and its propagation
    got = K.asr_conv0(xd, K.wave_stats(xd, AR.NORM_EPS), W[:, 0, :].t().contiguous().to(DEV), b.to(DEV), lg.to(DEV),
                      lb.to(DEV), s)
    assert got.shape == ((n - k) // s + 1, C)
    _check(f"asr_conv0 n{n} dc{dc}", got, AR.conv0(x, W, b, lg, lb, s), AR.conv0(x, W, b, lg, lb, s, emulate=True))


@pytest.mark.parametrize("T,d,groups,k", [(1, 128, 2, 128), (24, 128, 2, 128), (63, 128, 2, 128), (64, 128, 2, 128),
                                          (65, 128, 2, 128), (149, 128, 2, 128), (24, 1024, 16, 128),
                                          (24, 128, 2, 16), (24, 128, 2, 15),
                                          # the 128-position kernel under the widest halo (255 staged rows of the 264):
                                          # 2 position blocks x 128 groups = 256 blocks; the second block is ragged
                                          (200, 1024, 128, 128)])
def test_positional_conv(V, K, T, d, groups, k):
    g = _gen(T + d + k)
    cg = d // groups
    assert _splits(T, cg, cg, k, groups) == (groups < 128)
    h, W, b = torch.randn(T, d, generator=g), torch.randn(d, cg, k, generator=g) / (cg * k) ** 0.5, \
        0.1 * torch.randn(d, generator=g)
    wp = torch.cat([V.pack_conv_weight(W[i * cg:(i + 1) * cg]) for i in range(groups)]).to(DEV)
    hd = h.half().to(DEV)
    got = K.asr_conv(hd, wp, b.to(DEV), d, k, 1, k // 2, groups, T_out=T, res=hd)
    _check(f"pos_conv T{T} d{d} g{groups} k{k}", got, AR.pos_conv(h, W, b, groups), AR.pos_conv(h, W, b, groups, emulate=True))


def test_asr_conv_refuses_in_place(V, K):
    """Blocks read staged rows that other blocks write: out overlapping x is refused; res may be x."""
    h = torch.zeros(40, 64, dtype=torch.float16, device=DEV)
    wp = V.pack_conv_weight(torch.zeros(64, 64, 3)).to(DEV)
    with pytest.raises(ValueError, match="overlaps"):
        K.asr_conv(h, wp, None, 64, 3, 1, 1, out=h)
    with pytest.raises(ValueError, match="overlaps"):
        K.asr_conv(h, wp, None, 64, 3, 1, 1, T_out=20, res=h[:20], out=h[20:])
    assert K.asr_conv(h, wp, None, 64, 3, 1, 1, res=h).shape == (40, 64)


def _greedy_case(A, K, logits, lens, bias=None, blank=0):
    B, Tm, ld = logits.shape
    Vv = ld - 3                                     # the padded columns must be ignored
    ld_logits = logits.clone()
    ld_logits[:, :, Vv:] = 100.0
    lens32 = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    dev = ld_logits.to(DEV)
    ids, out, count, bad = K.ctc_greedy(dev, Vv, blank, lens32, None if bias is None else bias.to(DEV))
    full = logits[:, :, :Vv] + (0 if bias is None else bias)
    for b in range(B):
        T = Tm if lens is None else lens[b]
        assert torch.equal(dev[b, :T, :Vv].cpu(), full[b, :T])   # the bias is added in place, exactly
        want_ids = full[b, :T].argmax(1)
        assert torch.equal(ids[b, :T].cpu().long(), want_ids)
        want = A.collapse(want_ids.tolist(), blank)
        assert int(count[b]) == len(want) and out[b, :len(want)].tolist() == want
        assert int(bad[b]) == 0
    return count


def test_ctc_greedy_kernel(A, K):
    g = _gen(0)
    # integer logits in a narrow range: ties in most frames, runs and blanks everywhere
    ties = torch.randint(0, 3, (2, 1025, 11), generator=g).float()        # 1025 crosses the scan's 256-frame chunks
    _greedy_case(A, K, ties, None)
    _greedy_case(A, K, ties, [1025, 300], bias=torch.randint(0, 2, (8,), generator=g).float())
    _greedy_case(A, K, ties[:, :1].contiguous(), None)                     # T = 1
    _greedy_case(A, K, ties[:1, :257].contiguous(), [256])
    blank = torch.zeros(1, 700, 11)
    blank[:, :, 0] = 1.0
    assert int(_greedy_case(A, K, blank, None)[0]) == 0                    # all blank
    run = torch.zeros(1, 600, 11)
    run[:, :, 5] = 1.0
    assert int(_greedy_case(A, K, run, None)[0]) == 1                      # one run across the chunks
    alt = torch.zeros(1, 1025, 11)
    alt[0, torch.arange(1025), 1 + torch.arange(1025) % 2] = 1.0
    assert int(_greedy_case(A, K, alt, None)[0]) == 1025                   # every frame starts a run


def test_ctc_greedy_flags_non_finite(K):
    x = torch.zeros(3, 40, 8)
    x[1, 7, 2] = float("inf")
    x[2, 39, 1] = float("nan")                      # past lens[2]: not this utterance's logit
    bad = K.ctc_greedy(x.to(DEV), 8, 0, torch.tensor([40, 40, 39], dtype=torch.int32, device=DEV))[3]
    assert bad.tolist() == [0, 1, 0]


# ------------------------------------------------------------------------------------------ the model

@pytest.mark.parametrize("fx", AR.E2E_FIXTURES, ids=lambda f: f"{f[0]}-n{f[2]}-bias{f[4]}")
def test_end_to_end_small(A, fx):
    cfg_name, seed, n, wseed, bb = fx
    _, pcm, ref, emu = AR.reference(*fx)
    m = _model(A, cfg_name, seed, bb)
    x = AR.to_float(pcm)
    got = m.logits(x, sr=16000)
    allowance = _check(f"logits {fx}", got, ref, emu)
    sure = AR.margins(ref) >= 2 * allowance
    share = 1.0 - float(sure.float().mean())
    ids = got.argmax(1).cpu()
    print(f"  frames {ref.shape[0]}, excluded (margin < 2 x allowance) {share:.3f}, argmax equal on the rest: "
          f"{bool((ids[sure] == ref.argmax(1)[sure]).all())}")
    assert share <= AR.MARGIN_CAP
    assert torch.equal(ids[sure], ref.argmax(1)[sure])
    _, lens, dev_ids, _, _, _ = m.forward_batch([x])
    assert torch.equal(dev_ids[0, :lens[0]].cpu().long(), ids)
    text = m.transcribe(x)
    assert text == AR.decode(ids.tolist())
    print(f"  transcript: {text!r}")


BATCH = [("small", 0, 400, 4, 0.0), ("small", 0, 12345, 2, 0.0), ("small", 0, 48000, 3, 0.0)]


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)])
def test_transcribe_many_packed(A, order):
    """1, 38 and 149 frames in one packed encoder batch: key-length masking, a one-frame utterance; each
    utterance within allowance of its own one-at-a-time restatement, in either batch order."""
    m = _model(A, "small", 0)
    fxs = [BATCH[i] for i in order]
    waves = [AR.to_float(AR.reference(*fx)[1]) for fx in fxs]
    logits, lens, ids, out, count, bad = m.forward_batch(waves)
    assert lens == [AR.frame_count(fx[2]) for fx in fxs] and bad.tolist() == [0, 0, 0]
    texts = m.transcribe_many(waves, batch_size=3)
    for b, fx in enumerate(fxs):
        _, _, ref, emu = AR.reference(*fx)
        _check(f"packed {fx} at slot {b}", logits[b, :lens[b], :m.V], ref, emu)
        assert texts[b] == AR.decode(ids[b, :lens[b]].tolist())
    assert m.transcribe_many(waves, batch_size=1) == [m.transcribe(w) for w in waves]


def test_real_widths(A):
    """d 1024, 16 heads of 64, FFN 4096, 16 groups, conv width 512, two layers, 1 s of audio (49 frames)."""
    fx = ("wide", 0, 16000, 5, 0.0)
    _, pcm, ref, emu = AR.reference(*fx)
    assert ref.shape == (49, 32)
    _check(f"logits {fx}", _model(A, "wide", 0).logits(AR.to_float(pcm)), ref, emu)


def test_non_finite_guard(A):
    """A projection scaled far past fp16's range: the guard raises, no transcript comes back."""
    sd = dict(AR.make_state_dict(AR.SMALL, 0))
    sd["wav2vec2.feature_projection.projection.weight"] = sd["wav2vec2.feature_projection.projection.weight"] * 3e4
    m = A.Wav2Vec2CTC(sd, AR.SMALL, AR.VOCAB, device=DEV)
    x = AR.to_float(AR.make_wave(8000, 1))
    with pytest.raises(A.NonFiniteLogits, match="non-finite"):
        m.transcribe(x)
    with pytest.raises(A.NonFiniteLogits, match="non-finite"):
        m.logits(x)


def test_transcript_cli(A, tmp_path):
    """The CLI on an HF-layout directory of the small model and {i}_pred.wav files as the vocoder step writes
    them: one line per file in numeric order, equal to the host decode of the device's ids."""
    spec = importlib.util.spec_from_file_location("mms2ut_transcript", os.path.join(ROOT, "scripts", "mms2ut_transcript.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    sd = AR.make_state_dict(AR.SMALL, 0, blank_bias=2.0)
    AR.write_model_dir(str(tmp_path / "model"), sd, AR.SMALL, "safetensors")
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    V = pkg("vocoder")
    pcms = {i: AR.make_wave(n, 20 + i) for i, n in ((0, 9000), (2, 400), (10, 16000))}
    for i, pcm in pcms.items():
        V.write_wav(str(wavs / f"{i}_pred.wav"), torch.from_numpy(pcm.astype(np.float32) / 32767.0))
    out = tmp_path / "transcript.txt"
    assert cli.main(["--model-path", str(tmp_path / "model"), "--tts-wav-dir", str(wavs), "--transcript-txt", str(out),
                     "--batch-size", "2", "--device", DEV]) == 0
    m = _model(A, "small", 0, 2.0)
    want = []
    for group in ([0, 2], [10]):
        waves = [AR.to_float(pcms[i]) for i in group]
        _, lens, ids, _, _, _ = m.forward_batch(waves)
        want += [AR.decode(ids[b, :lens[b]].tolist()) for b in range(len(group))]
    lines = out.read_text().split("\n")
    print(f"transcripts: {lines}")
    assert lines == want and len(lines) == 3 and any(lines)
