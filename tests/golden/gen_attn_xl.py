"""Generate tests/golden/attn_xl.npz: ``AttentionXL.forward`` of the REAL reference (legacy/algorithm/modules/gtrxl.py, read-only
beside this repository) in float64 on three tiny seeded cases, with the gradients of sum(out * g).

Run (from the repo root):
    CUDA_VISIBLE_DEVICES="" PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:. python3 tests/golden/gen_attn_xl.py

Per case ``c<i>_``: the activations between the module's projections -- q, k, val (the two halves of attention_kv), r -- are
recorded by forward hooks on its own Linear layers, so that the restatement under test (tests/attn_xl_ref.py) starts where the HIP
kernel starts; ``project``'s weight and bias take its output back to the module's; the gradients with respect to q, k, val and r
are those of the hooked tensors under sum(y * gy), i.e. of sum(out * g) with g = gy W; du and dv those of the parameters.  The
mask is the one GTrXL.forward builds (gtrxl.py:423-427).  Arrays only."""
import os
import sys
from unittest import mock

import numpy as np

np.bool8 = np.bool_
for m in ["gym", "gym.spaces", "redis", "redis.backoff", "redis.retry", "wandb", "zmq", "blosc"]:
    sys.modules[m] = mock.MagicMock()
import torch

torch.set_num_threads(1)
from legacy.algorithm.modules.gtrxl import AttentionXL

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(2, 4, 3, 0, 2), (2, 4, 3, 4, 2), (3, 2, 1, 3, 1)]   # (nh, dh, C, M, N): causal; memory with C > 1; a rollout step


def main():
    out = {"cases": np.array(CASES, dtype=np.int64)}
    for ci, (nh, dh, C, M, N) in enumerate(CASES):
        torch.manual_seed(100 + ci)
        F, D = C + M, 10
        att = AttentionXL(D, dh, nh, torch.nn.Identity()).double()
        u, v = (torch.nn.Parameter(0.5 * torch.randn(nh, dh, dtype=torch.float64)) for _ in range(2))
        full = torch.randn(F, N, D, dtype=torch.float64)
        pos = torch.randn(F, 1, D, dtype=torch.float64)
        mask = torch.triu(torch.ones(C, F), diagonal=1 + M).bool().unsqueeze(-1)
        kept = {}

        def keep(name):
            def hook(_m, _i, y):
                y.retain_grad()
                kept[name] = y
            return hook

        for name, layer in (("kv", att.attention_kv), ("q", att.attention_q), ("r", att.project_pos)):
            layer.register_forward_hook(keep(name))
        y = att(full[M:], pos, full, u, v, mask=mask)
        gy = torch.randn(C, N, D, dtype=torch.float64)
        (y * gy).sum().backward()
        W = att.project.weight.detach()   # y = out W^T + b with out the attention vector: d out = gy W =: g
        kv, dkv = kept["kv"].detach(), kept["kv"].grad
        rec = dict(q=kept["q"].detach(), k=kv[..., :nh * dh], val=kv[..., nh * dh:], r=kept["r"].detach()[:, 0], u=u.detach(),
                   v=v.detach(), g=gy @ W, y=y.detach(), project_w=W, project_b=att.project.bias.detach(),
                   dq=kept["q"].grad, dk=dkv[..., :nh * dh], dval=dkv[..., nh * dh:], dr=kept["r"].grad[:, 0], du=u.grad, dv=v.grad)
        out.update({f"c{ci}_{n}": t.contiguous().numpy() for n, t in rec.items()})
    np.savez(os.path.join(HERE, "attn_xl.npz"), **out)


if __name__ == "__main__":
    main()
