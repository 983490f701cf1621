"""The front of a GTrXL layer restated in plain torch from its formulas (include/srl_hip.h, srl_gtrxl_qkv_fwd / _bwd), with the
backward in closed form (not autograd).  mem [M, N, D], x [C, N, D], keep [N] or None, gamma, beta [D], w_kv [2D, D], b_kv [2D],
w_q [D, D], b_q [D]; dkv [M + C, N, 2D], dq [C, N, D]."""
import torch

NAMES = ("mem", "x", "gamma", "beta", "w_kv", "b_kv", "w_q", "b_q")


def gtrxl_qkv(inputs, dkv, dq, dtype):
    """Returns kv, q, x1, stats = mean | rstd, dx, dgamma, dbeta, db_kv, db_q, dw_kv, dw_q in ``dtype``."""
    mem, x, gamma, beta, w_kv, b_kv, w_q, b_q = (inputs[n].to(dtype) for n in NAMES)
    dkv, dq, M, D = dkv.to(dtype), dq.to(dtype), mem.shape[0], x.shape[-1]
    keep = inputs.get("keep")
    full = torch.cat([mem if keep is None else mem * keep.to(dtype)[None, :, None], x])
    mean = full.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((full - mean) ** 2).mean(-1, keepdim=True) + 1e-5)
    xhat = (full - mean) * rstd
    x1 = xhat * gamma + beta
    dx1 = dkv @ w_kv
    g = dx1 * gamma
    dfull = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))   # (its memory rows go nowhere)
    return dict(kv=x1 @ w_kv.T + b_kv, q=x @ w_q.T + b_q, x1=x1, stats=torch.cat([mean, rstd], -1), dx=dfull[M:] + dq @ w_q,
                dgamma=(dx1 * xhat).sum((0, 1)), dbeta=dx1.sum((0, 1)), db_kv=dkv.sum((0, 1)), db_q=dq.sum((0, 1)),
                dw_kv=dkv.reshape(-1, 2 * D).T @ x1.reshape(-1, D), dw_q=dq.reshape(-1, D).T @ x.reshape(-1, D))
