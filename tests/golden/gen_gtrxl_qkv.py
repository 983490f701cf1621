"""Generate tests/golden/gtrxl_qkv.npz: the front of ``GatedTransformerXLLayer.forward`` / ``AttentionXL.forward`` of the REAL
reference (legacy/algorithm/modules/gtrxl.py, read-only beside this repository) -- cat, ``layernorm1``, ``attention.attention_kv``
on all rows, ``attention.attention_q`` on the inputs -- in float64 at D = 64, M = 3, C = 2, N = 5, the memory multiplied by
``1 - on_reset`` as ``AutoResetRNN.forward`` multiplies its state (batch row 1 is reset), with the autograd gradients of
sum(kv * dkv) + sum(q * dq).  The memory takes no gradient, as in the reference.

Run (from the repo root):
    CUDA_VISIBLE_DEVICES="" PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:. python3 tests/golden/gen_gtrxl_qkv.py

Records mem, x, keep, dkv, dq, the six parameters, kv, q, x1 and the gradients of x and of every parameter.  Arrays only."""
import os
import sys
from unittest import mock

import numpy as np

np.bool8 = np.bool_
for m in ["gym", "gym.spaces", "redis", "redis.backoff", "redis.retry", "wandb", "zmq", "blosc"]:
    sys.modules[m] = mock.MagicMock()
import torch

torch.set_num_threads(1)
from legacy.algorithm.modules.gtrxl import GatedTransformerXLLayer

HERE = os.path.dirname(os.path.abspath(__file__))
D, M, C, N = 64, 3, 2, 5


def main():
    torch.manual_seed(301)
    layer = GatedTransformerXLLayer(D, D // 4, D, 4, 2, torch.nn.Identity(), torch.nn.ReLU()).double()
    ln, att = layer.layernorm1, layer.attention
    with torch.no_grad():   # (a fresh LayerNorm is the identity map: give gamma and beta something to show)
        ln.weight.add_(0.3 * torch.randn(D, dtype=torch.float64))
        ln.bias.add_(0.3 * torch.randn(D, dtype=torch.float64))
    rn = lambda *s: torch.randn(*s, dtype=torch.float64)
    mem, x, dkv, dq = rn(M, N, D), rn(C, N, D).requires_grad_(), rn(M + C, N, 2 * D), rn(C, N, D)
    on_reset = torch.zeros(N, 1, dtype=torch.float64)
    on_reset[1] = 1
    masks = 1 - on_reset
    memory = mem * masks.reshape(1, N, 1)
    x1 = ln(torch.cat([memory, x], dim=0))
    kv, q = att.attention_kv(x1), att.attention_q(x)
    ((kv * dkv).sum() + (q * dq).sum()).backward()
    out = dict(mem=mem, x=x.detach(), keep=masks[:, 0], dkv=dkv, dq=dq, kv=kv.detach(), q=q.detach(), x1=x1.detach(), dx=x.grad)
    for name, p in (("gamma", ln.weight), ("beta", ln.bias), ("w_kv", att.attention_kv.weight), ("b_kv", att.attention_kv.bias),
                    ("w_q", att.attention_q.weight), ("b_q", att.attention_q.bias)):
        out[name], out["d" + name] = p.detach(), p.grad
    np.savez(os.path.join(HERE, "gtrxl_qkv.npz"), **{n: t.contiguous().numpy() for n, t in out.items()})


if __name__ == "__main__":
    main()
