"""R-Drop criterion, restated literally from fairseq's published source (test infrastructure).

fairseq ``RdropLabelSmoothedCrossEntropyCriterion`` (criterions/label_smoothed_cross_entropy_with_rdrop.py)
as the reference's ``speech_to_unit`` uses it (criterions/speech_to_speech_criterion.py:46-56,
:70-76): the net input is concatenated with itself, the label-smoothed CE is summed over all 2R
rows, and ``compute_kl_loss`` adds the symmetric KL of the two dropout passes:

    net_prob     = log_softmax(logits)            net_prob_tec = softmax(logits)
    p, q         = split(net_prob, R)             p_tec, q_tec = split(net_prob_tec, R)
    p_loss       = F.kl_div(p, q_tec, reduction="none")     # q_tec * (log q_tec - p)
    q_loss       = F.kl_div(q, p_tec, reduction="none")
    masked_fill_(pad_mask, 0) on both;  loss = (p_loss.sum() + q_loss.sum()) / 2

fairseq is not importable here, so this is not pinned against the library.  Everything runs in the
dtype of ``logits`` (the tests pass fp64, or fp32 to measure that format's own error); gradients
come from autograd.  ``closed_form`` is the algebra the HIP kernels implement.
"""
import torch
import torch.nn.functional as F

from fairseq_stub import _label_smoothed_nll_loss


def compute_kl_loss(lprobs, target_first_half, pad):
    """fairseq compute_kl_loss on log-probabilities [2R, V]; target_first_half [R]."""
    R = lprobs.shape[0] // 2
    probs = lprobs.exp()
    p, q = torch.split(lprobs, R, dim=0)
    p_tec, q_tec = torch.split(probs, R, dim=0)
    p_loss = F.kl_div(p, q_tec, reduction="none")
    q_loss = F.kl_div(q, p_tec, reduction="none")
    pad_mask = target_first_half.eq(pad).unsqueeze(-1)
    p_loss = p_loss.masked_fill(pad_mask, 0.0)
    q_loss = q_loss.masked_fill(pad_mask, 0.0)
    return (p_loss.sum() + q_loss.sum()) / 2


def rdrop_loss(logits, target_first_half, eps, pad, alpha):
    """logits [2R, V] (any float dtype, no pad columns), the first half's targets [R] ->
    (loss = CE over 2R rows + alpha * kl, nll over 2R rows, kl)."""
    lprobs = F.log_softmax(logits, dim=-1)
    target = torch.cat((target_first_half, target_first_half))
    ce, nll = _label_smoothed_nll_loss(lprobs, target, eps, ignore_index=pad, reduce=True)
    kl = compute_kl_loss(lprobs, target_first_half, pad)
    return ce + alpha * kl, nll, kl


def rdrop_loss_and_grad(logits, target_first_half, eps, pad, alpha, gloss=1.0):
    """(loss, nll, kl, d(gloss * loss)/d logits) by autograd, in the dtype of ``logits``."""
    z = logits.detach().clone().requires_grad_(True)
    loss, nll, kl = rdrop_loss(z, target_first_half, eps, pad, alpha)
    (loss * gloss).backward()
    return loss.detach(), nll.detach(), kl.detach(), z.grad


def closed_form(logits, target_first_half, eps, pad, alpha, gloss=1.0):
    """The closed forms of the issue (what the kernels compute), in the dtype of ``logits``:
    kl = 1/2 sum_r sum_v (p_v - q_v)(lp_v - lq_v); with d = lp - lq, K1 = sum p d, K2 = -sum q d:
    dkl/dz^p = 1/2 [p (d - K1) + p - q], dkl/dz^q = 1/2 [q (-d - K2) + q - p], zero on pad pairs,
    added to the CE gradient p - y_smooth.  -> (loss, nll, kl, gradient)."""
    R, V = logits.shape[0] // 2, logits.shape[1]
    lprobs = F.log_softmax(logits, dim=-1)
    lp, lq = lprobs[:R], lprobs[R:]
    p, q = lp.exp(), lq.exp()
    keep = target_first_half.ne(pad).unsqueeze(-1).to(logits.dtype)
    d = lp - lq
    kl = 0.5 * ((p - q) * d * keep).sum()
    K1 = (p * d).sum(-1, keepdim=True)
    K2 = -(q * d).sum(-1, keepdim=True)
    gkl = torch.cat((0.5 * (p * (d - K1) + p - q) * keep, 0.5 * (q * (-d - K2) + q - p) * keep))
    target = torch.cat((target_first_half, target_first_half))
    keep2 = torch.cat((keep, keep))
    eps_i = eps / (V - 1)
    safe = target.clamp(0, V - 1)
    onehot = F.one_hot(safe, V).to(logits.dtype)
    y = (1.0 - eps - eps_i) * onehot + eps_i           # the smoothed target distribution (sums to 1)
    gce = (lprobs.exp() - y) * keep2
    ce, nll = _label_smoothed_nll_loss(lprobs, target, eps, ignore_index=pad, reduce=True)
    return ce + alpha * kl, nll, kl, gloss * (gce + alpha * gkl)
