"""Generate tests/golden/gtrxl_gate.npz: ``GRUGatingUnit.forward`` of the REAL reference (legacy/algorithm/modules/gtrxl.py, read-only
beside this repository) in float64 at D = 64, rows = 5, random weights, bg = 2 + noise, with the autograd gradients of sum(g * dg).

Run (from the repo root):
    CUDA_VISIBLE_DEVICES="" PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:. python3 tests/golden/gen_gtrxl_gate.py

Records x, y, dg, the seven parameters under the module's own names, g, and d<name> for x, y and every parameter.  Arrays only."""
import os
import sys
from unittest import mock

import numpy as np

np.bool8 = np.bool_
for m in ["gym", "gym.spaces", "redis", "redis.backoff", "redis.retry", "wandb", "zmq", "blosc"]:
    sys.modules[m] = mock.MagicMock()
import torch

torch.set_num_threads(1)
from legacy.algorithm.modules.gtrxl import GRUGatingUnit

HERE = os.path.dirname(os.path.abspath(__file__))
D, ROWS = 64, 5


def main():
    torch.manual_seed(300)
    gate = GRUGatingUnit(D).double()
    with torch.no_grad():
        gate.bg.add_(0.1 * torch.randn(D, dtype=torch.float64))
    x, y = (torch.randn(ROWS, D, dtype=torch.float64, requires_grad=True) for _ in range(2))
    dg = torch.randn(ROWS, D, dtype=torch.float64)
    g = gate(x, y)
    (g * dg).sum().backward()
    out = dict(x=x.detach(), y=y.detach(), dg=dg, g=g.detach(), dx=x.grad, dy=y.grad)
    for name in ("Wr", "Wz", "Wg", "Ur", "Uz", "Ug"):
        out[name], out["d" + name] = getattr(gate, name).weight.detach(), getattr(gate, name).weight.grad
    out["bg"], out["dbg"] = gate.bg.detach(), gate.bg.grad
    np.savez(os.path.join(HERE, "gtrxl_gate.npz"), **{n: t.contiguous().numpy() for n, t in out.items()})


if __name__ == "__main__":
    main()
