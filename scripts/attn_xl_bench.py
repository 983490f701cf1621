"""Transformer-XL's relative attention (csrc/attn_xl.hip) against the same arithmetic composed from torch operators, on one GPU.

Three shapes (nh, dh, C, M, N): (4, 32, 32, 32, 4096), (4, 64, 16, 48, 4096) and the rollout step (4, 32, 1, 63, 4096).  Per shape:
forward and backward of the kernel (``hip.attn_xl_fwd`` / ``hip.attn_xl_bwd``, the fold launch included) and of the torch
composition (two bmm, the pad / view shift, masked_fill, softmax, bmm; its backward through autograd), device events around 10
calls, 9 repetitions, the two ways alternating; microseconds per call, median / min / max.  Also the kernel's byte floor -- q,
k, val read and out written once (backward: d out, q, k, val read, dq, dk, dval written) at 8 TB/s -- over the median, the torch /
kernel ratio, and the largest difference of the two outputs.  Prints one JSON line per shape; ``--out FILE`` writes them all.

    python scripts/attn_xl_bench.py [--out attn_xl_bench.json]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from srl_amd import hip

DEV, HBM_BYTES_PER_S = "cuda:0", 8e12
SHAPES = [(4, 32, 32, 32, 4096), (4, 64, 16, 48, 4096), (4, 32, 1, 63, 4096)]


def torch_attn(q, k, val, r, u, v, mask, nh, dh):
    """AttentionXL's arithmetic between its projections, operator for operator (bmm, pad / view shift, masked_fill, softmax, bmm)."""
    (C, N, _), F = q.shape, k.shape[0]
    qh = q.view(C, N, nh, dh)
    heads = lambda x: x.view(F, N, nh, dh).permute(1, 2, 0, 3).reshape(N * nh, F, dh)
    content = torch.bmm((qh + u).permute(1, 2, 0, 3).reshape(N * nh, C, dh), heads(k).transpose(1, 2))
    pos = ((qh + v).permute(1, 2, 0, 3) @ r.view(F, nh, dh).permute(1, 2, 0)).reshape(N * nh, C, F)
    pos = torch.nn.functional.pad(pos, [1, 0]).view(N * nh, F + 1, C)[:, 1:].reshape(N * nh, C, F)
    p = torch.softmax(((content + pos) * dh ** -0.5).masked_fill(mask, float("-inf")), dim=-1)
    return torch.bmm(p, heads(val)).view(N, nh, C, dh).permute(2, 0, 1, 3).reshape(C, N, nh * dh)


def timed(fns, reps=9, inner=10):
    times = {name: [] for name in fns}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner * 1e3)
    return {name: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v)) for name, v in times.items()}


def case(nh, dh, C, M, N):
    F, W, s = C + M, nh * dh, dh ** -0.25
    g = torch.Generator().manual_seed(1)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(DEV)
    q, kv, r, u, v, dout = s * rn(C, N, W), rn(F, N, 2 * W), s * rn(F, W), 0.5 * s * rn(nh, dh), 0.5 * s * rn(nh, dh), rn(C, N, W)
    kv[..., :W] *= s
    out, lse = torch.empty(C, N, W, device=DEV), torch.empty(N, nh, C, device=DEV)
    dq, dkv, dr, du, dv = torch.empty_like(q), torch.empty_like(kv), torch.empty_like(r), torch.empty_like(u), torch.empty_like(v)
    ws = torch.empty(hip.attn_xl_bwd_workspace(nh, dh, C, M, N) // 4, device=DEV)
    kp, dkp = kv.data_ptr(), dkv.data_ptr()

    def k_fwd():
        hip.attn_xl_fwd(q.data_ptr(), W, kp, kp + 4 * W, 2 * W, r.data_ptr(), W, u.data_ptr(), v.data_ptr(), N, nh, dh, C, M,
                        out.data_ptr(), W, lse.data_ptr())

    def k_bwd():
        hip.attn_xl_bwd(dout.data_ptr(), W, q.data_ptr(), W, kp, kp + 4 * W, 2 * W, r.data_ptr(), W, u.data_ptr(), v.data_ptr(),
                        lse.data_ptr(), N, nh, dh, C, M, dq.data_ptr(), W, dkp, dkp + 4 * W, 2 * W, dr.data_ptr(), W, du.data_ptr(),
                        dv.data_ptr(), ws.data_ptr(), ws.numel() * 4)

    mask = torch.triu(torch.ones(C, F, device=DEV), diagonal=1 + M).bool()
    leaves = [x.clone().requires_grad_() for x in (q, kv, r, u, v)]
    t_fwd = lambda: torch_attn(leaves[0], leaves[1][..., :W], leaves[1][..., W:], *leaves[2:], mask, nh, dh)
    y = t_fwd()

    def t_bwd():
        torch.autograd.grad(y, leaves, dout, retain_graph=True)

    k_fwd()
    torch.cuda.synchronize()
    rec = timed({"kernel_fwd": k_fwd, "torch_fwd": lambda: t_fwd().detach(), "kernel_bwd": k_bwd, "torch_bwd": t_bwd})
    rec["max_abs_out_diff"] = float((out - y.detach()).abs().max())
    for d, rows in (("fwd", 2 * C + 2 * F), ("bwd", 3 * C + 4 * F)):   # [N, nh dh] float32 rows moved once
        floor_us = rows * N * W * 4 / HBM_BYTES_PER_S * 1e6
        rec[f"{d}_byte_floor_us"] = floor_us
        rec[f"{d}_fraction_of_floor"] = floor_us / rec[f"kernel_{d}"]["median_us"]
        rec[f"{d}_torch_over_kernel"] = rec[f"torch_{d}"]["median_us"] / rec[f"kernel_{d}"]["median_us"]
    print(json.dumps({"shape": [nh, dh, C, M, N], **rec}), flush=True)
    return rec


if __name__ == "__main__":
    assert torch.cuda.is_available()
    res = {"-".join(map(str, sh)): case(*sh) for sh in SHAPES}
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)
