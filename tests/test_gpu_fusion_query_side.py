"""The query-side form of the gated fusion's one-head attention (csrc/layers.hip): S = scale (q W_k)
X^T, O = (Pd X) W_v^T, with b_k / b_v / bias_kv as tail columns of the augmented weights.

Each form is forced with mms2ut_gated_fusion_set_route and compared with the fp32 CPU oracle
(oracle/ref_model.py fuse_img_feat) under the bounds tests/test_gpu_model.py uses for the fusion:
result relative L2 error < 5e-3, text gradient < 1e-2, parameter gradients < 2e-2, and the
"k_proj bias gradient vanishes" bound of the selective attention.  The image gradient (want_dimg)
is a data gradient through the same chain as the text gradient and takes the text-gradient bound.
"""
import pytest
import torch

from conftest import pkg
from oracle import ref_model as R

pytestmark = pytest.mark.gpu

D = 128
MMA, SA = "multimodal_attention", "selective_attention"
RES_TOL, DATA_TOL, PARAM_TOL = 5e-3, 1e-2, 2e-2


@pytest.fixture(scope="module")
def mm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m = pkg()
    yield m
    m.kernels.fusion_set_route(-1)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _params(ocfg, seed):
    """fp16-representable fusion parameters; every bias (and the LayerNorm) moved off its init so
    b_k, b_v and bias_kv carry weight in the result."""
    g = torch.Generator().manual_seed(seed)
    P = {k: v for k, v in R.init_params(ocfg, seed=seed, include_unused=False).items()
         if k.startswith(("encoder.selective", "encoder.multimodal", "encoder.gate", "encoder.image"))}
    for k, v in P.items():
        if v.dim() == 1 or k.endswith((".bias_k", ".bias_v")):
            P[k] = v + 0.2 * torch.randn(v.shape, generator=g)
    return {k: v.half().float() for k, v in P.items()}


def _case(mm, route, att=MMA, gate=True, B=3, Te=5, Ti=7, Di=128, mask=False, want_dimg=False, drops=(0.0, 0.0, 0.0),
          seed=0, d=D, per_launch=False):
    """One forward + backward of the HIP fusion under `route` (per_launch: model.fusion_*_ref, one
    launch at a time from Python) -> its outputs (CPU) and the inputs."""
    K = mm.kernels
    p_img, p_txt, p_att = drops
    cfg = mm.default_cfg(encoder_embed_dim=d, encoder_layers=0, decoder_layers=0, image_feat_dim=Di,
                         encoder_attention_heads=1, multimodal_attention_type=att, use_selective_gate=gate,
                         SA_image_dropout=p_img, SA_text_dropout=p_txt, SA_attention_dropout=p_att, conv_channels=16,
                         decoder_embed_dim=d, decoder_attention_heads=1, vocab_size=8)
    ocfg = R.base_config(encoder_embed_dim=d, image_feat_dim=Di, multimodal_attention_type=att, use_selective_gate=gate,
                         SA_image_dropout=p_img, SA_text_dropout=p_txt, SA_attention_dropout=p_att)
    P = _params(ocfg, 11 + seed)
    model = mm.MMS2UTModel(cfg, device="cuda")
    model.params.load_state_dict(P, strict=False)
    model.drop.reset(99)
    g = torch.Generator().manual_seed(seed)
    text = torch.randn(B * Te, d, generator=g).half()
    img = torch.randn(B, Ti, Di, generator=g).half()
    gout = torch.randn(B * Te, d, generator=g).half()
    Tk = Ti + (att == MMA)
    km = None
    if mask:
        km = torch.zeros(B, (Ti + 1 + 7) // 8 * 8, dtype=torch.uint8)
        for b in range(B):
            km[b, Ti - (2 * b + 1) % Ti:Ti] = 1     # a different number of padded keys per utterance
    K.fusion_set_route(route)
    try:
        assert model._fusion_call(Di).route(B, Te, Ti) == route
        fwd, bwd = (model.fusion_fwd_ref, model.fusion_bwd_ref) if per_launch else (model.fusion_fwd, model.fusion_bwd)
        res, c = fwd(text.cuda(), img.cuda(), None if km is None else km.cuda(), B, Te)
        out = bwd(c, gout.cuda(), want_dimg=want_dimg)
        K.side_join()
        torch.cuda.synchronize()
    finally:
        K.fusion_set_route(-1)
    dtext, dimg = out if want_dimg else (out, None)
    grads = {k: model.params.g[k].float().cpu().clone() for k in P}
    masks = None
    if p_img or p_txt or p_att:
        masks = {"fusion.img": K.dropout_mask(B * Ti * Di, p_img, *c["drop_img"], "cuda").view(B, Ti, Di).transpose(0, 1).cpu().bool(),
                 "fusion.txt": K.dropout_mask(B * Te * d, p_txt, *c["drop_txt"], "cuda").view(B, Te, d).transpose(0, 1).cpu().bool(),
                 "fusion.attn": K.dropout_mask(B * Te * Tk, p_att, *c["drop_attn"], "cuda").view(B, Te, Tk).cpu().bool()}
    return {"res": res.float().cpu(), "dtext": dtext.float().cpu(), "dimg": None if dimg is None else dimg.float().cpu(),
            "grads": grads, "P": P, "text": text, "img": img, "gout": gout, "km": km, "masks": masks, "ocfg": ocfg,
            "dims": (B, Te, Ti, Di, d), "route": route}


def _oracle(r):
    B, Te, Ti, Di, d = r["dims"]
    Pg = {k: v.clone().requires_grad_(True) for k, v in r["P"].items()}
    t_o = r["text"].float().view(B, Te, d).transpose(0, 1).clone().requires_grad_(True)
    i_o = r["img"].float().transpose(0, 1).clone().requires_grad_(True)
    km = None if r["km"] is None else r["km"][:, :Ti].bool()
    ro = R.fuse_img_feat(Pg, t_o, i_o, km, None, r["ocfg"], r["masks"])
    (ro * r["gout"].float().view(B, Te, d).transpose(0, 1)).sum().backward()
    return ro.detach(), t_o.grad, i_o.grad, Pg


def _check(r, oracle=None):
    """The bounds of tests/test_gpu_model.py on the result, the text (and image) gradient and every
    parameter gradient.  For the query-side form the packed in-projection bias is checked per
    q / k / v third, so b_k and b_v each meet the bound on their own.  The key-side form (unchanged
    code) keeps the granularity tests/test_gpu_model.py pins it at, the whole vector: its b_k third
    is the column sum of fp16 dK rows that cancel to -dS[:, Ti] (about sqrt(B Ti) 2^-11 |dK| of
    rounding against a near-zero sum; 2.7e-2 measured at Ti = 100 with an image key mask)."""
    B, Te, Ti, Di, d = r["dims"]
    ro, gt, gi, Pg = oracle or _oracle(r)
    errs = {"res": (rel(r["res"], ro.transpose(0, 1).reshape(B * Te, d)), RES_TOL),
            "dtext": (rel(r["dtext"], gt.transpose(0, 1).reshape(B * Te, d)), DATA_TOL)}
    if r["dimg"] is not None:
        errs["dimg"] = (rel(r["dimg"], gi.transpose(0, 1).reshape(B * Ti, Di)), DATA_TOL)
    for k, v in Pg.items():
        if v.grad is None:
            assert ".gate_denses." in k and not r["ocfg"]["use_selective_gate"], k
            continue
        g = r["grads"][k]
        if k.endswith("selective_attns.0.k_proj.bias"):   # mathematically zero (shift-invariant softmax)
            bound = 1e-2 * Pg[k.replace("k_proj", "v_proj")].grad.norm().item() + 1e-3
            errs[k] = (g.norm().item(), bound)
        elif k.endswith(".in_proj_bias") and r["route"] == 1:
            for i, n in enumerate("qkv"):
                errs[f"{k}[{n}]"] = (rel(g[i * d:(i + 1) * d], v.grad[i * d:(i + 1) * d]), PARAM_TOL)
        else:
            errs[k] = (rel(g.view(v.grad.shape), v.grad), PARAM_TOL)
    print({k: f"{e:.2e}" for k, (e, _) in errs.items()})
    bad = {k: e for k, e in errs.items() if not e[0] < e[1]}
    assert not bad, bad
    return len(errs)


@pytest.mark.parametrize("Di", [128, 256, 320])
@pytest.mark.parametrize("Ti", [7, 100])
@pytest.mark.parametrize("Te", [5, 17])
def test_query_side_matches_oracle(mm, Te, Ti, Di):
    """B = 3, d = 128: Tk = Ti + 1 is no multiple of 8; Di = d, Di != d, and Di % 256 != 0 (the
    unfused LayerNorm path).  Multimodal attention: b_k, b_v, bias_k and bias_v all enter."""
    n = _check(_case(mm, 1, Te=Te, Ti=Ti, Di=Di, seed=Te + Ti + Di))
    assert n >= 12    # res, dtext, LN w/b, in-proj weight(s), 3 bias thirds, bias_k, bias_v, out-proj w/b, gate w/b


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("att,gate,mask,want_dimg,Di", [
    (SA, True, False, False, 256),
    (SA, False, False, False, 320),
    (MMA, False, False, False, 128),
    (MMA, True, True, False, 256),       # image key mask, a different count per utterance
    (SA, True, True, False, 128),
    (MMA, True, False, True, 256),       # image gradient through the fused LayerNorm backward
    (SA, True, False, True, 320),        # ... and through the unfused one
])
def test_variants_match_oracle(mm, route, att, gate, mask, want_dimg, Di):
    _check(_case(mm, route, att=att, gate=gate, Te=17, Ti=100 if mask else 7, Di=Di, mask=mask, want_dimg=want_dimg,
                 seed=3))


@pytest.mark.parametrize("att", [MMA, SA])
def test_query_side_dropout_replay_vs_oracle(mm, att):
    """Dropout on (image 0.3, text 0.2, attention 0.1): the HIP RNG's masks replayed in the oracle,
    as tests/test_gpu_model.py test_fusion_dropout_replay_vs_oracle does for the key-side form."""
    _check(_case(mm, 1, att=att, Te=9, Ti=17, Di=256, drops=(0.3, 0.2, 0.1), seed=5))


def test_route_rule(mm):
    """The cost rule: ViT features at the benchmark's shape take the query-side form, DETR features
    with long text the key-side one."""
    def route(Di, Te, Ti):
        cfg = mm.default_cfg(encoder_embed_dim=768, encoder_layers=0, decoder_layers=0, image_feat_dim=Di,
                             encoder_attention_heads=1, conv_channels=16, decoder_embed_dim=768,
                             decoder_attention_heads=1, vocab_size=8)
        return mm.MMS2UTModel(cfg, device="cuda")._fusion_call(Di).route(8, Te, Ti)
    mm.kernels.fusion_set_route(-1)
    assert route(768, 106, 577) == 1
    assert route(256, 200, 100) == 0


def test_forms_agree(mm):
    """Both forms, same inputs and dropout masks: within the oracle bounds of each other."""
    kw = dict(Te=17, Ti=100, Di=256, mask=True, want_dimg=True, drops=(0.3, 0.2, 0.1), seed=7)
    a, b = _case(mm, 0, **kw), _case(mm, 1, **kw)
    assert rel(b["res"], a["res"]) < RES_TOL
    assert rel(b["dtext"], a["dtext"]) < DATA_TOL and rel(b["dimg"], a["dimg"]) < DATA_TOL
    for k, g in a["grads"].items():
        assert rel(b["grads"][k], g) < PARAM_TOL, k


def test_query_side_deterministic(mm):
    kw = dict(Te=17, Ti=100, Di=320, mask=True, want_dimg=True, drops=(0.3, 0.2, 0.1), seed=9)
    a, b = _case(mm, 1, **kw), _case(mm, 1, **kw)
    assert torch.equal(a["res"], b["res"]) and torch.equal(a["dtext"], b["dtext"]) and torch.equal(a["dimg"], b["dimg"])
    for k, g in a["grads"].items():
        assert torch.equal(g, b["grads"][k]), k


@pytest.mark.parametrize("att,Di", [(MMA, 256), (SA, 320)])
def test_query_side_one_call_equals_per_launch(mm, att, Di):
    """The per-launch restatement (model.fusion_fwd_ref / fusion_bwd_ref) issues the query-side
    form's kernels in the library's order: same bits (tests/test_gpu_layers.py's property, here with
    the route forced, dropout on, an image key mask and the image gradient)."""
    kw = dict(att=att, Te=17, Ti=100, Di=Di, mask=True, want_dimg=True, drops=(0.3, 0.2, 0.1), seed=13)
    a, b = _case(mm, 1, **kw), _case(mm, 1, per_launch=True, **kw)
    assert torch.equal(a["res"], b["res"]) and torch.equal(a["dtext"], b["dtext"]) and torch.equal(a["dimg"], b["dimg"])
    for k, g in a["grads"].items():
        assert torch.equal(g, b["grads"][k]), k


@pytest.mark.parametrize("B,Te", [(1, 5), (3, 1), (1, 1)])
def test_query_side_single_row(mm, B, Te):
    _check(_case(mm, 1, B=B, Te=Te, Ti=7, Di=128, seed=B + Te))
