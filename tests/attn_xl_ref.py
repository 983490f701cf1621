"""Transformer-XL's relative attention restated in plain torch from its formula (include/srl_hip.h, srl_attn_xl_fwd): per batch
row and head, C current steps over F = M + C keys,
    s[i, j] = dh^-0.5 ((q[i] + u) . k[j] + (q[i] + v) . r[j + C - 1 - i])   for j <= i + M, else -inf;   out = softmax_j(s) val.
q [C, N, nh dh]; k, val [F, N, nh dh]; r [F, nh dh]; u, v [nh, dh]."""
import torch

NAMES = ("q", "k", "val", "r", "u", "v")


def attn_xl(q, k, val, r, u, v):
    (C, N, _), F, (nh, dh) = q.shape, k.shape[0], u.shape
    qh, kh, vh, rh = q.view(C, N, nh, dh), k.view(F, N, nh, dh), val.view(F, N, nh, dh), r.view(F, nh, dh)
    i, j = torch.arange(C)[:, None], torch.arange(F)[None, :]
    t = torch.einsum("inhd,mhd->nhim", qh + v, rh)
    # (under the mask j + C - 1 - i runs past F - 1: any in-range index will do there)
    pos = t.gather(3, (j + C - 1 - i).clamp(max=F - 1).expand(N, nh, C, F))
    s = (torch.einsum("inhd,jnhd->nhij", qh + u, kh) + pos) * dh ** -0.5
    p = torch.softmax(s.masked_fill(j > i + (F - C), float("-inf")), dim=-1)
    return torch.einsum("nhij,jnhd->inhd", p, vh).reshape(C, N, nh * dh)


def attn_xl_grads(inputs, g, dtype):
    """``inputs``: name -> tensor for NAMES; returns {"out", "dq", "dk", "dval", "dr", "du", "dv"} of sum(out * g) in ``dtype``."""
    x = [inputs[n].detach().to(dtype).requires_grad_() for n in NAMES]
    out = attn_xl(*x)
    grads = torch.autograd.grad((out * g.to(dtype)).sum(), x)
    return dict(out=out.detach(), **{"d" + n: t for n, t in zip(NAMES, grads)})
