"""GPU: the speech-to-unit kernels (csrc/units.hip, asr_conv's GELU epilogue and its 48-channel groups) and
the HubertUnits forward built on them, against the fp32 CPU restatement in tests/hubert_ref.py.

Tolerances are measured, not chosen (the convention of tests/test_gpu_asr.py): a GPU result may be at most
TOL_FACTOR (3) x as far from the fp32 restatement (max-abs) as the restatement's own fp16-storage emulation
is for the same inputs; every check prints its floor and ratio.  Units are compared on the frames that
hubert_ref.safe_frames calls safe for that allowance; tests/test_units.py bounds the share of the others.
kmeans_assign itself is compared with a float64 evaluation of |C|^2 - 2 x . C on the same fp16 rows: it
must agree wherever the float64 top-2 gap exceeds TOL_FACTOR x the distance of a torch emulation of its
rounding from float64, and at most 1 % of the rows may have a smaller gap (the centroids carry 22 bits)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import asr_ref as AR
import hubert_ref as HR
from conftest import ROOT, pkg
from conv_dispatch import splits as _splits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def U():
    return pkg("units")


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
    assert floor > 0 and err <= HR.TOL_FACTOR * floor, (name, err, floor)
    return HR.TOL_FACTOR * floor


# ------------------------------------------------------------------------------------------ layer 0

@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("n", [25, 400, 719, 8000, 160000])
def test_groupnorm_layer0(K, n, C):
    """4 frames and 79 frames (fewer than the statistics' 256 parts), unused trailing samples, many blocks,
    every part busy (31999 frames, 125 per part); a DC offset of 0.4 on a 0.2-rms signal; with and without
    the input normalisation and the bias.  The statistics against float64 on the same (fp32-normalised)
    samples; a mean is measured on its channel's scale max(|mean|, std), as a channel whose taps sum to
    nearly 0 has a mean near 0.  Measured: mean <= 5.9e-8, rstd <= 6.0e-8 (the rounding of the results to fp32)."""
    k, s = 10, 5
    g = _gen(n + C)
    x = AR.to_float(AR.make_wave(n, n, dc=0.4))
    W, b = torch.randn(C, 1, k, generator=g) / k ** 0.5, 0.1 * torch.randn(C, generator=g)
    gg, gb = 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    xd, wd = x.to(DEV), W[:, 0, :].t().contiguous().to(DEV)
    T0 = (n - k) // s + 1
    for normalize in (False, True):
        st = K.wave_stats(xd, AR.NORM_EPS) if normalize else None
        for bias in (None, b):
            args = (xd, st, wd, None if bias is None else bias.to(DEV), gg.to(DEV), gb.to(DEV), s)
            got, mr = K.hubert_conv0(*args, return_stats=True)
            assert got.shape == (T0, C)
            _check(f"hubert_conv0 n{n} C{C} norm{normalize} bias{bias is not None}", got,
                   HR.conv0(x, W, bias, gg, gb, s, normalize=normalize),
                   HR.conv0(x, W, bias, gg, gb, s, normalize=normalize, emulate=True))
            xn = x if st is None else (x - st.cpu()[0]) * st.cpu()[1]        # the kernel's own fp32 samples
            v = torch.nn.functional.conv1d(xn.double()[None, None], W.double(), None if bias is None else bias.double(),
                                           stride=s)[0]
            mean, var = v.mean(1), v.var(1, unbiased=False)
            rstd = 1.0 / torch.sqrt(var + HR.GN_EPS)
            scale = torch.maximum(mean.abs(), var.sqrt())
            e_mean = float(((mr[:, 0].cpu().double() - mean).abs() / scale).max())
            e_rstd = float(((mr[:, 1].cpu().double() - rstd).abs() / rstd).max())
            print(f"  statistics vs float64: mean {e_mean:.2e}, rstd {e_rstd:.2e} (relative)")
            assert e_mean <= 1e-6 and e_rstd <= 1e-6
            again, mr2 = K.hubert_conv0(*args, return_stats=True)
            assert torch.equal(again, got) and torch.equal(mr2, mr)          # bitwise reproducible


def test_hubert_conv0_refuses_bad_shapes(K):
    x = torch.zeros(100, device=DEV)
    w, g = torch.zeros(10, 64, device=DEV), torch.ones(64, device=DEV)
    with pytest.raises(ValueError, match="fewer"):
        K.hubert_conv0(x[:5].contiguous(), None, w, None, g, g, 5)
    with pytest.raises(pkg("_lib").HipError, match="stride"):
        K.hubert_conv0(x, None, w, None, g, g, 17)
    with pytest.raises(pkg("_lib").HipError, match="channels"):
        K.hubert_conv0(x, None, torch.zeros(10, 520, device=DEV), None, torch.ones(520, device=DEV),
                       torch.ones(520, device=DEV), 5)


# ------------------------------------------------------------------------------------------ asr_conv

@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("T,Cin,Cout,k,s,split", [
    (37, 64, 64, 3, 2, True),        # odd T: the trailing row is unused
    (130, 64, 72, 2, 2, True),       # Cout off the 64-grid: a second, narrow channel block
    (8195, 512, 512, 3, 2, False)])  # the real width on the 128-position kernel, one output in the last block
def test_conv_gelu_epilogue(V, K, T, Cin, Cout, k, s, split, with_bias):
    assert _splits((T - k) // s + 1, Cin, Cout, k) == split
    g = _gen(T + Cin)
    x, W = torch.randn(T, Cin, generator=g), 1.6 * torch.randn(Cout, Cin, k, generator=g) / (Cin * k) ** 0.5
    b = 0.1 * torch.randn(Cout, generator=g) if with_bias else None
    got = K.asr_conv(x.half().to(DEV), V.pack_conv_weight(W).to(DEV), None if b is None else b.to(DEV), Cout, k, s,
                     gelu=True)
    assert got.shape[0] == (T - k) // s + 1
    _check(f"asr_conv+GELU {Cin}->{Cout} k{k} s{s} T{T} bias{with_bias}", got, HR.conv_gelu(x, W, b, s),
           HR.conv_gelu(x, W, b, s, emulate=True))


def test_conv_gelu_keyword_excludes_res(V, K):
    h = torch.zeros(40, 64, dtype=torch.float16, device=DEV)
    wp = V.pack_conv_weight(torch.zeros(64, 64, 3)).to(DEV)
    with pytest.raises(ValueError, match="gelu"):
        K.asr_conv(h, wp, None, 64, 3, 1, 1, res=h, gelu=True)


@pytest.mark.parametrize("T,d,groups,k", [(1, 768, 16, 128), (49, 768, 16, 128), (149, 768, 16, 128),
                                          (200, 768, 16, 128), (24, 96, 2, 128), (24, 96, 2, 15)])
def test_positional_conv_48_per_group(V, K, T, d, groups, k):
    """48 channels per group (HuBERT-base: d 768, 16 groups): three of a block's four 16-channel tiles in
    use, and slices of 48 input channels, so a 32-wide K-step straddles two taps."""
    g = _gen(T + d + k)
    cg = d // groups
    assert cg == 48 and _splits(T, cg, cg, k, groups)
    h, W, b = torch.randn(T, d, generator=g), torch.randn(d, cg, k, generator=g) / (cg * k) ** 0.5, \
        0.1 * torch.randn(d, generator=g)
    wp = torch.cat([V.pack_conv_weight(W[i * cg:(i + 1) * cg]) for i in range(groups)]).to(DEV)
    hd = h.half().to(DEV)
    got = K.asr_conv(hd, wp, b.to(DEV), d, k, 1, k // 2, groups, T_out=T, res=hd)
    _check(f"pos_conv T{T} d{d} g{groups} k{k}", got, AR.pos_conv(h, W, b, groups), AR.pos_conv(h, W, b, groups, emulate=True))


# ------------------------------------------------------------------------------------------ kmeans_assign

def _km_inputs(R, d, Kc, seed):
    """Rows that sit among the centroids: a centroid each plus noise of half its spread."""
    g = _gen(seed)
    Cm = torch.randn(Kc, d, generator=g)
    X = (Cm[torch.randint(0, Kc, (R,), generator=g)] + 0.5 * torch.randn(R, d, generator=g)).half()
    return X, Cm


def _km_check(K, name, X3, Cm, lens=None):
    """kmeans_assign on X3 fp16 [B, Tm, d] at both chunk widths against float64 -> code of the default run."""
    B, Tm, d = X3.shape
    packed = tuple(t.to(DEV) for t in K.kmeans_pack(Cm))
    lens32 = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    rows = X3.reshape(B * Tm, d)
    S = HR.scores(rows.float(), Cm)                                   # float64, the same fp16 rows
    valid = (torch.ones(B, Tm, dtype=torch.bool) if lens is None else
             torch.arange(Tm)[None] < torch.tensor(lens)[:, None]).reshape(-1)
    allow = HR.TOL_FACTOR * float((HR.kmeans_emulation(rows, Cm).double() - S)[valid].abs().max())
    top = S.topk(min(2, Cm.shape[0]), dim=1, largest=False).values
    gap = top[:, 1] - top[:, 0] if Cm.shape[0] > 1 else torch.full((B * Tm,), float("inf"), dtype=torch.float64)
    sure = (gap > allow) & valid
    share = 1.0 - float(sure[valid].float().mean())
    out = None
    for chunk in (None, 256):
        code, merged, count, bad = K.kmeans_assign(X3.to(DEV), *packed, lens32, chunk=chunk)
        assert K.kmeans_chunks(B * Tm, Cm.shape[0], chunk)[0] == (chunk or 64)     # few rows: 64 centroids per block
        c = code.cpu().reshape(-1).long()
        ok = bool((c[sure] == S.argmin(1)[sure]).all())
        print(f"{name} chunk {chunk or 64}: allowance {allow:.3e}, rows under it {share:.4f}, argmin equal on the rest: {ok}")
        assert ok and share <= 0.01 and bad.tolist() == [0] * B
        for b in range(B):
            T = Tm if lens is None else lens[b]
            want = HR.merge(code[b, :T].tolist())
            assert int(count[b]) == len(want) and merged[b, :len(want)].tolist() == want
            assert not code[b, T:].any()                               # rows past the length get no code
        again = K.kmeans_assign(X3.to(DEV), *packed, lens32, chunk=chunk)
        assert all(torch.equal(a, b_) for a, b_ in zip(again, (code, merged, count, bad)))   # bitwise reproducible
        if out is not None:
            assert torch.equal(out, code)                              # the chunking changes nothing
        out = code
    return out


@pytest.mark.parametrize("R,d,Kc", [(1, 128, 1), (1, 128, 16), (149, 128, 100), (257, 768, 1000), (300, 1024, 1000),
                                    (70, 72, 130)])          # the last: d off the 32-grid, Kc off the 64- and 16-grids
def test_kmeans_assign_kernel(K, R, d, Kc):
    X, Cm = _km_inputs(R, d, Kc, R + d + Kc)
    _km_check(K, f"kmeans_assign R{R} d{d} Kc{Kc}", X[None], Cm)


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)])
def test_kmeans_assign_packed(K, order):
    """1, 38 and 149 frames in one packed batch, in either order, finite garbage in the padding rows."""
    lens = [(1, 38, 149)[i] for i in order]
    X, Cm = _km_inputs(3 * 149, 128, 100, 7)
    X3 = X.reshape(3, 149, 128).clone()
    for b, T in enumerate(lens):
        X3[b, T:] = 1000.0
    _km_check(K, f"kmeans_assign packed {lens}", X3, Cm, lens)


def test_kmeans_assign_ties_and_tail(K):
    g = _gen(3)
    Cm = 2.0 * torch.randn(100, 128, generator=g)             # 100 centroids: images of 112 rows, chunks of 64
    Cm[7] = Cm[3]                                             # exact duplicates: the lower index wins
    Cm[70] = Cm[3]                                            # ... also across the chunk boundary
    X = torch.cat([Cm[3][None].repeat(5, 1), torch.zeros(1, 128), Cm[99][None]]).half()
    hi, lo, cn = (t.to(DEV) for t in K.kmeans_pack(Cm))
    hi[100:], lo[100:] = 1.0, -1.0                            # the padded rows: anything finite
    assert float(cn.min()) > 0                                # the row at the origin scores |C|^2 > 0 everywhere real,
    want_origin = int(cn.argmin())                            # a padded lane with a zero norm would score 0 and win
    for chunk in (None, 256):
        code, merged, count, bad = K.kmeans_assign(X[None].to(DEV), hi, lo, cn, chunk=chunk)
        assert code[0].tolist() == [3] * 5 + [want_origin, 99]
        assert merged[0, :3].tolist() == [3, want_origin, 99] and count.tolist() == [3] and bad.tolist() == [0]


def test_kmeans_merge_known_answers(K):
    """Rows that are centroids themselves: the codes are known.  A single-frame utterance, one long run across
    the scan's 256-frame chunks, alternating units (every frame starts a run)."""
    Cm = 4.0 * torch.randn(20, 64, generator=_gen(5)).half().float()
    packed = tuple(t.to(DEV) for t in K.kmeans_pack(Cm))
    Tm = 600
    seqs = [[11], [5] * 600, [i % 2 + 8 for i in range(513)], [0, 0, 19, 19, 19, 0, 4]]
    X3 = torch.zeros(len(seqs), Tm, 64, dtype=torch.float16)
    for b, sq in enumerate(seqs):
        X3[b, :len(sq)] = Cm[sq].half()
    lens = torch.tensor([len(sq) for sq in seqs], dtype=torch.int32, device=DEV)
    code, merged, count, bad = K.kmeans_assign(X3.to(DEV), *packed, lens)
    assert bad.tolist() == [0] * 4 and count.tolist() == [1, 1, 513, 4]
    for b, sq in enumerate(seqs):
        assert code[b, :len(sq)].tolist() == sq
        assert merged[b, :int(count[b])].tolist() == HR.merge(sq)
    assert merged[3, :4].tolist() == [0, 19, 0, 4]


def test_kmeans_flags_non_finite(K):
    X, Cm = _km_inputs(3 * 40, 64, 30, 9)
    X3 = X.reshape(3, 40, 64).clone()
    X3[1, 7, 2] = float("inf")                      # a value, not a fault: the fp16 overflow of an activation
    X3[2, 39, 1] = float("inf")                     # past lens[2]: not this utterance's row
    packed = tuple(t.to(DEV) for t in K.kmeans_pack(Cm))
    bad = K.kmeans_assign(X3.to(DEV), *packed, torch.tensor([40, 40, 39], dtype=torch.int32, device=DEV))[3]
    assert bad.tolist() == [0, 1, 0]
    X3[0, 0, :] = float("nan")
    bad = K.kmeans_assign(X3.to(DEV), *packed, torch.tensor([40, 40, 39], dtype=torch.int32, device=DEV))[3]
    assert bad.tolist() == [1, 1, 0]


# ------------------------------------------------------------------------------------------ the model

_MODELS = {}


def _model(U, cfg_name, normalize=False):
    key = (cfg_name, normalize)
    if key not in _MODELS:
        cfg = HR.CFGS[cfg_name]
        _MODELS[key] = U.HubertUnits(HR.make_state_dict(cfg, 0), cfg, HR.make_centroids(cfg_name).numpy(),
                                     HR.KM_LAYER[cfg_name], {"do_normalize": normalize}, device=DEV)
    return _MODELS[key]


def _units_check(name, ref, allowance, code):
    cents = HR.make_centroids("small")
    safe = HR.safe_frames(ref, cents, allowance)
    share = 1.0 - float(safe.float().mean())
    want = HR.assign(ref, cents)
    code = torch.as_tensor(code).long()
    print(f"  {name}: frames {ref.shape[0]}, unsafe {share:.3f}, units equal on the rest: "
          f"{bool((code[safe] == want[safe]).all())}, distinct {code.unique().numel()}")
    assert share <= HR.MARGIN_CAP
    assert torch.equal(code[safe], want[safe])


@pytest.mark.parametrize("n,ws", HR.WAVES)
@pytest.mark.parametrize("normalize", [False, True])
def test_end_to_end_small(U, n, ws, normalize):
    _, pcm, ref, emu = HR.reference("small", n, ws, normalize=normalize)
    m = _model(U, "small", normalize)
    x = AR.to_float(pcm)
    feats = m.features(x, sr=16000)
    allowance = _check(f"features n{n} normalize{normalize}", feats, ref, emu)
    code, merged = m.units(x)
    assert len(code) == ref.shape[0] and merged == HR.merge(code)
    if not normalize:
        _units_check(f"n{n}", ref, allowance, code)


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)])
def test_units_many_packed(U, order):
    """1, 38 and 149 frames in one packed batch: key-length masking, no padding in a convolution or in the
    GroupNorm statistics; each utterance within allowance of its own one-at-a-time restatement."""
    m = _model(U, "small")
    fxs = [[(400, 4), (12345, 2), (48000, 3)][i] for i in order]
    refs = [HR.reference("small", n, ws) for n, ws in fxs]
    waves = [AR.to_float(r[1]) for r in refs]
    Fb, lens, code, merged, count, bad = m.forward_batch(waves)
    assert lens == [AR.frame_count(n) for n, _ in fxs] and bad.tolist() == [0, 0, 0]
    res = m.units_many(waves, batch_size=3)
    for b, (_, _, ref, emu) in enumerate(refs):
        allowance = _check(f"packed {fxs[b]} at slot {b}", Fb[b, :lens[b]], ref, emu)
        if lens[b] > 1:       # tests/test_units.py bounds the unsafe share of the 38- and 149-frame fixtures
            _units_check(f"slot {b}", ref, allowance, res[b][0])
        assert res[b][0] == code[b, :lens[b]].tolist() and res[b][1] == HR.merge(res[b][0])
    assert m.units_many(waves, batch_size=1) == [m.units(w) for w in waves]


def test_real_widths(U):
    """conv 512, d 768, 12 heads of 64, FFN 3072, 16 groups of 48, two layers, 1000 centroids; 1 s of audio."""
    _, pcm, ref, emu = HR.reference("wide", 16000, 5)
    assert ref.shape == (49, 768)
    m = _model(U, "wide")
    feats = m.features(AR.to_float(pcm))
    _check("features wide", feats, ref, emu)
    code, merged = m.units(AR.to_float(pcm))
    cents = HR.make_centroids("wide")
    S = HR.scores(feats.float().cpu(), cents)                 # on the device's own features: the quantiser alone
    allow = HR.TOL_FACTOR * float((HR.kmeans_emulation(feats.cpu(), cents).double() - S).abs().max())
    top = S.topk(2, dim=1, largest=False).values
    sure = (top[:, 1] - top[:, 0]) > allow
    print(f"  units wide: allowance {allow:.3e}, rows above it {float(sure.float().mean()):.3f}, distinct "
          f"{len(set(code))}")
    assert sure.float().mean() >= 0.9 and torch.equal(torch.tensor(code)[sure], S.argmin(1)[sure])
    assert merged == HR.merge(code)


def test_non_finite_guard(U):
    """A projection scaled far past fp16's range: the guard raises, no units come back."""
    sd = dict(HR.make_state_dict(HR.SMALL, 0))
    sd["feature_projection.projection.weight"] = sd["feature_projection.projection.weight"] * 3e4
    m = U.HubertUnits(sd, HR.SMALL, HR.make_centroids("small").numpy(), 2, device=DEV)
    with pytest.raises(U.NonFiniteFeatures, match="non-finite"):
        m.units(AR.to_float(AR.make_wave(8000, 1)))


def test_quantize_cli(U, tmp_path):
    """The CLI on an HF-layout directory of the small model, a .npy centroid file and a manifest: one line per
    file in manifest order, equal to the model's own units; --reduce writes the collapsed units."""
    import json
    spec = importlib.util.spec_from_file_location("mms2ut_quantize_units", os.path.join(ROOT, "scripts", "mms2ut_quantize_units.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(HR.SMALL))
    AR.write_safetensors(str(mdir / "model.safetensors"), HR.make_state_dict(HR.SMALL, 0, prefix="hubert."))
    np.save(tmp_path / "km.npy", HR.make_centroids("small").numpy())
    root = tmp_path / "audio"
    root.mkdir()
    pcms = {"b": AR.make_wave(9000, 21), "a": AR.make_wave(400, 22), "c": AR.make_wave(16000, 23)}
    for nm, pcm in pcms.items():
        AR.write_wav(str(root / f"{nm}.wav"), pcm)
    (tmp_path / "m.tsv").write_text(f"{root}\n" + "".join(f"{nm}.wav\t{len(p)}\n" for nm, p in pcms.items()))
    m = _model(U, "small")
    want = m.units_many([AR.to_float(p) for p in list(pcms.values())[:2]], 2) + m.units_many([AR.to_float(pcms["c"])], 2)
    for reduce in (False, True):
        out = tmp_path / f"out{int(reduce)}.km"
        assert cli.main(["--feature_type", "hubert", "--acoustic_model_path", str(mdir), "--kmeans_model_path",
                         str(tmp_path / "km.npy"), "--layer", "2", "--manifest_path", str(tmp_path / "m.tsv"),
                         "--out_quantized_file_path", str(out), "--batch-size", "2", "--device", DEV]
                        + (["--reduce"] if reduce else [])) == 0
        lines = out.read_text().splitlines()
        assert lines == [f"{nm}|" + " ".join(map(str, w[int(reduce)])) for nm, w in zip(pcms, want)]
    print(f"units: {lines}")
