"""GTrXL's GRU-style gating unit restated in plain torch from its formulas (include/srl_hip.h, srl_gtrxl_gate_fwd / _bwd), with the
backward in closed form (not autograd).  x, y, dg [rows, D]; w_y = Wr | Wz | Wg and w_x = Ur | Uz | Ug, [3D, D] each; bg [D]."""
import torch

NAMES = ("x", "y", "w_y", "w_x", "bg")


def gtrxl_gate(inputs, dg, dtype):
    """Returns g, gates = r | z | h, dx, dy, A = a_r | a_z | a_g, rx, d_bg, dw_y, dw_x in ``dtype``."""
    x, y, w_y, w_x, bg = (inputs[n].to(dtype) for n in NAMES)
    dg, D = dg.to(dtype), x.shape[1]
    pre = y @ w_y.T
    r = torch.sigmoid(pre[:, :D] + x @ w_x[:D].T)
    z = torch.sigmoid(pre[:, D:2 * D] + x @ w_x[D:2 * D].T - bg)
    rx = r * x
    h = torch.tanh(pre[:, 2 * D:] + rx @ w_x[2 * D:].T)
    g = (1 - z) * x + z * h
    a_g = dg * z * (1 - h * h)
    a_z = dg * (h - x) * z * (1 - z)
    t = a_g @ w_x[2 * D:]
    A = torch.cat([t * x * r * (1 - r), a_z, a_g], dim=1)
    dx = dg * (1 - z) + t * r + A[:, :2 * D] @ w_x[:2 * D]
    dw_x = torch.cat([A[:, :2 * D].T @ x, a_g.T @ rx])
    return dict(g=g, gates=torch.cat([r, z, h], dim=1), dx=dx, dy=A @ w_y, A=A, rx=rx, d_bg=-a_z.sum(0), dw_y=A.T @ y, dw_x=dw_x)
