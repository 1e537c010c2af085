"""GPU: the unit vocoder's kernels (csrc/vocoder.hip) and the CodeHiFiGAN forward built on them, against
the fp32 CPU restatement in tests/vocoder_ref.py.

Tolerances are measured, not chosen: a GPU result may be at most TOL_FACTOR (3) x as far from the fp32
restatement (max-abs) as the restatement's own fp16-storage emulation is for the same inputs.  The
duration predictor is fp32 on the GPU, so its durations are compared for equality.

conv1d_tm's block owns 128 output positions, or 32 where its waves split the reduction (at least
4 K-steps of 32 and fewer than 256 blocks of 128: csrc/conv1d_tm.h conv_splits), so the lengths
"just past one and two tiles" are 129 and 257, and 33 for the short tile; 1 and 7 are shorter than the
largest halo, d (k - 1) / 2 = 25.  Of CONV_SHAPES, 16->16 k3 and 8->8 k3 (2 and 1 K-steps) take the
128-position kernel and the others the 32-position one; test_conv1d_tm_block_count_threshold
crosses the block-count side of the rule."""
import pytest
import torch

import vocoder_ref as VR
from conftest import pkg
from conv_dispatch import splits as _splits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def V():
    return pkg("vocoder")


@pytest.fixture(scope="module")
def K():
    return pkg("kernels")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _check(name, got, ref, emu):
    """got within TOL_FACTOR x the emulation's distance from the fp32 restatement."""
    floor = float((emu - ref).abs().max())
    err = float((got.float().cpu() - ref).abs().max())
    print(f"{name}: emulation floor {floor:.3e}, GPU error {err:.3e} ({err / floor if floor else float('nan'):.2f}x)")
    assert torch.isfinite(got).all()
    assert floor > 0 and err <= VR.TOL_FACTOR * floor, (name, err, floor)


# ------------------------------------------------------------------------------------------ conv1d_tm

CONV_SHAPES = [(16, 16, 3, 1), (16, 16, 11, 5), (32, 32, 7, 3), (128, 64, 7, 1), (64, 64, 11, 1),
               (8, 8, 3, 3), (24, 40, 5, 2)]          # the last two: the narrowest width, widths off the 16-grid
CONV_T = [1, 7, 33, 129, 257]
# the epilogues the generator issues: conv_pre; a ResBlock's first conv; its second conv; the last
# second conv of a stage's first / later ResBlocks (scaled set / scaled accumulate)
EPILOGUES = {
    "plain": dict(),
    "in_out_lrelu": dict(in_slope=0.1, out_slope=0.1),
    "in_lrelu": dict(in_slope=0.1),
    "residual": dict(res=True),
    "residual_set": dict(res=True, scale=1.0 / 3, acc="set"),
    "residual_add": dict(res=True, scale=1.0 / 3, acc="add"),
    "out_lrelu_add": dict(out_slope=0.1, scale=0.5, acc="add"),
}


def _conv_case(V, K, Cin, Cout, k, dil, T, epi, seed=0):
    L = pkg("_lib")
    g = _gen(seed + 1000 * T + Cin)
    x, W, b = torch.randn(T, Cin, generator=g), torch.randn(Cout, Cin, k, generator=g) / (Cin * k) ** 0.5, \
        0.1 * torch.randn(Cout, generator=g)
    res = torch.randn(T, Cout, generator=g) if epi.get("res") else None
    prev = torch.randn(T, Cout, generator=g) if epi.get("acc") == "add" else None
    kw = dict(in_slope=epi.get("in_slope"), res=res, out_slope=epi.get("out_slope"), scale=epi.get("scale"), prev=prev)
    ref, emu = VR.conv_tm(x, W, b, dil, **kw), VR.conv_tm(x, W, b, dil, emulate=True, **kw)
    out = prev.half().to(DEV) if prev is not None else None
    acc = {None: L.VOC_ACC_NONE, "set": L.VOC_ACC_SET, "add": L.VOC_ACC_ADD}[epi.get("acc")]
    got = K.conv1d_tm(x.half().to(DEV), V.pack_conv_weight(W).to(DEV), b.to(DEV), Cout, k, dil,
                      in_slope=epi.get("in_slope"), res=None if res is None else res.half().to(DEV),
                      out_slope=epi.get("out_slope"), acc=acc, scale=epi.get("scale") or 1.0, out=out)
    assert tuple(got.shape) == (T, Cout)
    return got, ref, emu


@pytest.mark.parametrize("T", CONV_T)
@pytest.mark.parametrize("Cin,Cout,k,dil", CONV_SHAPES)
def test_conv1d_tm(V, K, Cin, Cout, k, dil, T):
    got, ref, emu = _conv_case(V, K, Cin, Cout, k, dil, T, {})
    _check(f"conv1d_tm {Cin}->{Cout} k{k} d{dil} T{T}", got, ref, emu)


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("Cin,Cout,k,dil,T", [(32, 32, 7, 3, 257), (16, 16, 11, 5, 7)])
def test_conv1d_tm_epilogues(V, K, Cin, Cout, k, dil, T, epi):
    got, ref, emu = _conv_case(V, K, Cin, Cout, k, dil, T, EPILOGUES[epi], seed=7)
    _check(f"conv1d_tm {epi} {Cin}->{Cout} k{k} d{dil} T{T}", got, ref, emu)


@pytest.mark.parametrize("T", [128 * 255, 128 * 255 + 1])
def test_conv1d_tm_block_count_threshold(V, K, T):
    """255 blocks of 128 positions: the waves split K (4 K-steps); 256: they split the positions."""
    got, ref, emu = _conv_case(V, K, 16, 16, 7, 1, T, EPILOGUES["residual_add"], seed=3)
    _check(f"conv1d_tm 16->16 k7 T{T}", got, ref, emu)


@pytest.mark.parametrize("Cin,Cout,k,dil,T", [(512, 16, 11, 5, 40), (128, 64, 7, 1, 128 * 256 + 5), (200, 24, 3, 2, 50)])
def test_conv1d_tm_channel_slices(V, K, Cin, Cout, k, dil, T):
    """The input channels pass through LDS in 64-wide slices: eight of them under the widest halo
    (32-position kernel), two in the 128-position kernel (256 blocks), and 200 channels, whose last
    slice is 8 wide."""
    got, ref, emu = _conv_case(V, K, Cin, Cout, k, dil, T, EPILOGUES["in_out_lrelu"], seed=5)
    _check(f"conv1d_tm {Cin}->{Cout} k{k} d{dil} T{T}", got, ref, emu)


def test_conv1d_tm_strided_rows(V, K):
    """Input, residual and output as column slices of wider buffers (row strides above the width)."""
    g = _gen(11)
    T, C, k = 131, 16, 3
    x, W, b, res = torch.randn(T, C, generator=g), torch.randn(C, C, k, generator=g) / (C * k) ** 0.5, \
        torch.randn(C, generator=g), torch.randn(T, C, generator=g)
    ref, emu = VR.conv_tm(x, W, b, res=res), VR.conv_tm(x, W, b, res=res, emulate=True)
    xb, rb = torch.zeros(T, 48, dtype=torch.float16, device=DEV), torch.zeros(T, 24, dtype=torch.float16, device=DEV)
    ob = torch.full((T, 32), 7.0, dtype=torch.float16, device=DEV)
    xb[:, 16:32], rb[:, 8:24] = x.half().to(DEV), res.half().to(DEV)
    K.conv1d_tm(xb[:, 16:32], V.pack_conv_weight(W).to(DEV), b.to(DEV), C, k, res=rb[:, 8:24], out=ob[:, 8:24])
    _check("conv1d_tm strided", ob[:, 8:24], ref, emu)
    assert (ob[:, :8] == 7).all() and (ob[:, 24:] == 7).all()


@pytest.mark.parametrize("Cin,Cout", [(12, 16), (16, 20), (4, 8)])
def test_conv1d_tm_rejects_widths(V, K, Cin, Cout):
    L = pkg("_lib")
    x = torch.zeros(9, Cin, dtype=torch.float16, device=DEV)
    w = torch.zeros(4096, dtype=torch.float16, device=DEV)
    with pytest.raises(L.HipError, match="multiples of 8"):
        K.conv1d_tm(x, w, None, Cout, 3)


@pytest.mark.parametrize("T,Cin,Cout,split", [
    (33, 64, 64, True),              # 6 K-steps: the 32-position kernel, a ragged second block
    (129, 16, 16, False),            # 2 K-steps: the 128-position kernel, a ragged second block
    (40, 128, 72, True)])            # 12 K-steps over two Cin slices; Cout off the 64-grid
def test_asr_conv_and_conv1d_tm_are_one_tile(V, K, T, Cin, Cout, split):
    """asr_conv at stride 1 and conv1d_tm at dilation 1 are the same convolution through the same tile
    (csrc/conv1d_tm.h): the same reduction in the same order and one rounding of acc + bias, so the two
    entry points agree bit for bit."""
    assert _splits(T, Cin, Cout, 3) == split
    g = _gen(T + Cin)
    x = torch.randn(T, Cin, generator=g).half().to(DEV)
    w = V.pack_conv_weight(torch.randn(Cout, Cin, 3, generator=g) / (Cin * 3) ** 0.5).to(DEV)
    b = (0.1 * torch.randn(Cout, generator=g)).to(DEV)
    a, v = K.asr_conv(x, w, b, Cout, 3, stride=1, pad=1), K.conv1d_tm(x, w, b, Cout, 3)
    assert tuple(a.shape) == tuple(v.shape) == (T, Cout) and bool(v.abs().max() > 0)
    assert torch.equal(a, v)


# ------------------------------------------------------------------------------------------ conv_transpose1d_tm

@pytest.mark.parametrize("T", [1, 3, 67])
@pytest.mark.parametrize("Cin,Cout", [(32, 16), (64, 32)])
@pytest.mark.parametrize("k,u", [(11, 5), (8, 4), (4, 2)])
def test_conv_transpose1d_tm(V, K, k, u, Cin, Cout, T):
    g = _gen(100 * k + T + Cin)
    p = (k - u) // 2
    x, W, b = torch.randn(T, Cin, generator=g), torch.randn(Cin, Cout, k, generator=g) * (u / (Cin * k)) ** 0.5, \
        0.1 * torch.randn(Cout, generator=g)
    ref = VR.conv_transpose_tm(x, W, b, u, p, in_slope=0.1)
    emu = VR.conv_transpose_tm(x, W, b, u, p, in_slope=0.1, emulate=True)
    got = K.conv_transpose1d_tm(x.half().to(DEV), V.pack_conv_transpose_weight(W, u).to(DEV), b.to(DEV), Cout, k, u, p,
                                in_slope=0.1)
    assert tuple(got.shape) == ((T - 1) * u - 2 * p + k, Cout) == tuple(ref.shape)
    _check(f"conv_transpose1d_tm k{k} u{u} {Cin}->{Cout} T{T}", got, ref, emu)


def test_conv_transpose1d_tm_two_tiles_no_activation(V, K):
    """More than one block per phase (T + taps - 1 > 128), no input activation, no bias."""
    g = _gen(5)
    T, Cin, Cout, k, u, p = 140, 16, 8, 8, 4, 2
    x, W = torch.randn(T, Cin, generator=g), torch.randn(Cin, Cout, k, generator=g) * (u / (Cin * k)) ** 0.5
    ref, emu = VR.conv_transpose_tm(x, W, None, u, p), VR.conv_transpose_tm(x, W, None, u, p, emulate=True)
    got = K.conv_transpose1d_tm(x.half().to(DEV), V.pack_conv_transpose_weight(W, u).to(DEV), None, Cout, k, u, p)
    assert tuple(got.shape) == (T * u, Cout)
    _check("conv_transpose1d_tm two tiles", got, ref, emu)


# ------------------------------------------------------------------------------------------ conv_post, gather

@pytest.mark.parametrize("Cin,T", [(8, 1), (16, 5), (16, 300), (8, 257)])
def test_conv_post_tanh(K, Cin, T):
    g = _gen(T + Cin)
    x, W, b = 2 * torch.randn(T, Cin, generator=g), torch.randn(1, Cin, 7, generator=g) / (Cin * 7) ** 0.5, \
        0.1 * torch.randn(1, generator=g)
    ref, emu = VR.conv_post_tanh(x, W, b), VR.conv_post_tanh(x, W, b, emulate=True)
    got = K.conv_post_tanh(x.half().to(DEV), W[0].t().contiguous().to(DEV), float(b[0]), 3, VR.POST_SLOPE)
    assert got.dtype == torch.float32 and tuple(got.shape) == (T,)
    _check(f"conv_post_tanh Cin{Cin} T{T}", got, ref, emu)


@pytest.mark.parametrize("D", [128, 8])
def test_embed_repeat_exact(K, D):
    g = _gen(3)
    table = torch.randn(50, D, generator=g).half()
    codes = torch.randint(0, 50, (23,), generator=g)
    dur = torch.tensor([1, 1, 3, 1, 40, 37, 50, 64, 1, 2, 1, 1, 9, 1, 1, 1, 5, 1, 1, 30, 1, 1, 1])
    assert dur.numel() == codes.numel() and int(dur.min()) == 1
    cum = torch.cumsum(dur, 0)
    got = K.embed_repeat(table.to(DEV), codes.to(DEV), cum.to(DEV), int(cum[-1]))
    want = VR.embed_repeat(table, codes, dur)
    assert tuple(got.shape) == (int(dur.sum()), D) and torch.equal(got.cpu(), want)
    assert torch.equal(K.embed_repeat(table.to(DEV), codes.to(DEV)).cpu(), table[codes])


# ------------------------------------------------------------------------------------------ the model

def _model(V, cfg, seed):
    sd = VR.make_state_dict(cfg, seed=seed)
    return sd, V.CodeHiFiGAN(sd, cfg, device=DEV)


@pytest.fixture(scope="module")
def small(V):
    return _model(V, VR.SMALL, 0)


def _codes(T, seed):
    return torch.randint(0, 1000, (T,), generator=_gen(seed))


def test_duration_predictor_matches_reference(small):
    sd, voc = small
    codes = _codes(121, 4)                                  # 31 blocks of 4 frames, the last one ragged
    e, dur_ref = VR.duration_predictor(sd, VR.SMALL, codes)
    keep = VR.away_from_boundary(e)
    assert float(keep.float().mean()) >= 0.95               # the CPU reference alone: the seed's property
    assert int(dur_ref.min()) == 1 and int(dur_ref.max()) >= 3     # the clamp and real rounding both occur
    logd, dur = voc.durations(codes)
    assert dur.dtype == torch.int32 and tuple(dur.shape) == (121,)
    print(f"duration predictor: {int(keep.sum())} of 121 frames kept, max |logd - ref| "
          f"{float((logd.cpu() - torch.log(e + 1)).abs().max()):.2e}")
    assert torch.equal(dur.cpu().long()[keep], dur_ref[keep])


@pytest.mark.parametrize("dur_prediction", [False, True])
def test_end_to_end_small(small, dur_prediction):
    sd, voc = small
    codes = _codes(37, 0)
    dur = None
    if dur_prediction:
        e, dur = VR.duration_predictor(sd, VR.SMALL, codes)
        assert VR.away_from_boundary(e).all()               # every frame is safe: equal lengths are required
        assert torch.equal(voc.durations(codes)[1].cpu().long(), dur)
    ref, peak = VR.forward(sd, VR.SMALL, codes, dur)
    emu, _ = VR.forward(sd, VR.SMALL, codes, dur, emulate=True)
    assert peak < VR.ACT_LIMIT
    got = voc.synthesize(codes, dur_prediction=dur_prediction)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape) == ((int(dur.sum()) if dur_prediction else 37) * 40,)
    _check(f"end to end small dur={dur_prediction}", got, ref, emu)
    assert voc.launches == 2 + 3 * 19 + 1 + (2 if dur_prediction else 0)


def test_end_to_end_released_shape(V):
    cfg = {k: v for k, v in VR.RELEASED.items() if k != "dur_predictor_params"}
    sd, voc = _model(V, cfg, 1)
    codes = _codes(20, 1)
    ref, peak = VR.forward(sd, cfg, codes)
    emu, _ = VR.forward(sd, cfg, codes, emulate=True)
    assert peak < VR.ACT_LIMIT
    got = voc.synthesize(codes)
    assert tuple(got.shape) == (6400,) == tuple(ref.shape)
    _check("end to end released shape T20", got, ref, emu)
    assert voc.launches == 98
    with pytest.raises(ValueError, match="duration predictor"):
        voc.synthesize(codes, dur_prediction=True)


def test_deterministic_and_many(small):
    _, voc = small
    utts = [_codes(37, 0), _codes(5, 2), _codes(1, 3)]
    a = [voc.synthesize(c, dur_prediction=True) for c in utts]
    b = voc.synthesize_many([c.tolist() for c in utts], dur_prediction=True)
    c = [voc.synthesize(c, dur_prediction=True) for c in utts]
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    # one library call for the whole generator == one call per kernel, bit for bit
    for u in utts:
        for dp in (False, True):
            one = voc.synthesize(u, dur_prediction=dp)
            n = voc.launches
            assert torch.equal(one, voc.synthesize_stepwise(u, dur_prediction=dp)) and voc.launches == n
    with pytest.raises(ValueError, match="unit code"):
        voc.synthesize([3, 1000])


def test_generate_waveform_script(V, tmp_path):
    """scripts/mms2ut_generate_waveform.py: unit file in, 16 kHz {i}_pred.wav out, equal to synthesize()."""
    import importlib.util
    import json
    import os
    M = pkg("manifest")
    sd, voc = _model(V, VR.SMALL, 0)
    torch.save({"generator": sd}, tmp_path / "model.pt")
    (tmp_path / "config.json").write_text(json.dumps(VR.SMALL))
    (tmp_path / "codes.txt").write_text("5 5 17 900\n3 999 0 0 0 12 44\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mms2ut_generate_waveform",
                                                  os.path.join(root, "scripts", "mms2ut_generate_waveform.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "wav"
    mod.main(["--in-code-file", str(tmp_path / "codes.txt"), "--vocoder", str(tmp_path / "model.pt"), "--vocoder-cfg",
              str(tmp_path / "config.json"), "--results-path", str(out), "--dur-prediction"])
    for i, codes in enumerate(([5, 5, 17, 900], [3, 999, 0, 0, 0, 12, 44])):
        x, sr = M.read_wav(str(out / f"{i}_pred.wav"))
        want = voc.synthesize(codes, dur_prediction=True).cpu().numpy().astype("float64")
        assert sr == 16000 and x.shape == want.shape
        assert (x == (want * 32767.0).round().clip(-32768, 32767)).all()
