"""The front of a GTrXL layer (csrc/gtrxl_qkv.hip) against the same arithmetic from torch operators and against the library's own
composition, on one GPU.

Three shapes (D, M, C, N): (256, 64, 16, 1024), (128, 64, 16, 2048) and the rollout step (256, 64, 1, 4096).  Per shape, forward and
backward (the fold launch included, the weight gradients on no side) of
  kernel   ``hip.gtrxl_qkv_fwd`` saving x1 and stats / ``hip.gtrxl_qkv_bwd``;
  torch    mul, cat, F.layer_norm, two F.linear; its backward through autograd with respect to x and the six parameters;
  pieces   the masked copy and the concatenation (torch, into a buffer that exists), ``hip.layernorm_fwd``, two ``hip.gemm`` /
           two ``hip.gemm`` in the data-gradient form, ``hip.layernorm_bwd`` over all rows, two ``hip.colsum``.
Device events around 10 calls, 9 repetitions, the three ways alternating; microseconds per call, median / min / max.  Also both
ratios over the kernel, the kernel's float32-matrix flop floor ((4 F + 2 C) N D^2 flops per direction at 157.3 TFLOP/s) and its
byte floor (forward mem, x read, kv, q, x1 written; backward dkv, dq, mem, x read, dx written; once, at 8 TB/s), each over the
median, and the largest difference between the kernel's and torch's kv, q and dx.  Prints one JSON line per shape; ``--out FILE``
writes them all.

    python scripts/gtrxl_qkv_bench.py [--out gtrxl_qkv_bench.json]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from srl_amd import hip

DEV, HBM_BYTES_PER_S, F32_MATRIX_FLOPS = "cuda:0", 8e12, 157.3e12
SHAPES = [(256, 64, 16, 1024), (128, 64, 16, 2048), (256, 64, 1, 4096)]


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


def case(D, M, C, N):
    g = torch.Generator().manual_seed(1)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(DEV)
    Fs, rows, cur = M + C, (M + C) * N, C * N
    mem, x, dkv, dq = rn(M, N, D), rn(C, N, D), rn(Fs, N, 2 * D), rn(C, N, D)
    keep = (torch.rand(N, generator=g) > 0.1).float().to(DEV)
    gamma, beta, w_kv, b_kv, w_q, b_q = 1 + 0.3 * rn(D), 0.3 * rn(D), D ** -0.5 * rn(2 * D, D), 0.1 * rn(2 * D), D ** -0.5 * rn(D, D), 0.1 * rn(D)
    e = lambda *sh: torch.empty(*sh, device=DEV)
    kv, q, x1, stats, dx, sums = e(Fs, N, 2 * D), e(C, N, D), e(Fs, N, D), e(rows, 2), e(C, N, D), e(5 * D)
    ws = e(hip.gtrxl_qkv_bwd_workspace(D, rows) // 4)
    P = lambda t: t.data_ptr()

    def k_fwd():
        hip.gtrxl_qkv_fwd(P(mem), D, P(x), D, P(keep), P(gamma), P(beta), P(w_kv), P(b_kv), P(w_q), P(b_q), M, C, N, D, P(kv), 2 * D, P(q), D,
                          P(x1), D, P(stats))

    def k_bwd():
        hip.gtrxl_qkv_bwd(P(dkv), 2 * D, P(dq), D, P(mem), D, P(x), D, P(keep), P(stats), P(gamma), P(w_kv), P(w_q), M, C, N, D, P(dx), D,
                          P(sums), P(sums) + 4 * D, P(sums) + 8 * D, P(sums) + 16 * D, P(ws), ws.numel() * 4)

    leaves = [t.clone().requires_grad_() for t in (x, gamma, beta, w_kv, b_kv, w_q, b_q)]

    def t_fwd():
        xl, ga, be, wk, bk, wq, bq = leaves
        full = torch.cat([mem * keep[None, :, None], xl])
        return F.linear(F.layer_norm(full, (D,), ga, be), wk, bk), F.linear(xl, wq, bq)

    ref = t_fwd()
    t_bwd = lambda: torch.autograd.grad(ref, leaves, [dkv, dq], retain_graph=True)

    full, y1, mean, rstd, kv2, q2, dx1, dfull, sums2 = e(Fs, N, D), e(Fs, N, D), e(rows), e(rows), e(Fs, N, 2 * D), e(C, N, D), e(rows, D), e(rows, D), e(5 * D)

    def p_fwd():
        torch.mul(mem, keep[None, :, None], out=full[:M])
        full[M:].copy_(x)
        hip.layernorm_fwd(P(full), D, P(gamma), P(beta), rows, D, P(y1), D, P(mean), P(rstd))
        hip.gemm(rows, 2 * D, D, P(y1), D, 0, P(w_kv), D, 0, P(kv2), 2 * D, bias=P(b_kv))
        hip.gemm(cur, D, D, P(x), D, 0, P(w_q), D, 0, P(q2), D, bias=P(b_q))

    def p_bwd():   # (dgamma / dbeta are added to by the library's LayerNorm backward: the same work; dx = dfull's current rows)
        hip.gemm(rows, D, 2 * D, P(dkv), 2 * D, 0, P(w_kv), D, 1, P(dx1), D)
        hip.layernorm_bwd(P(dx1), D, P(full), D, P(gamma), P(mean), P(rstd), rows, D, P(dfull), D, 0, P(sums2), P(sums2) + 4 * D)
        hip.gemm(cur, D, D, P(dq), D, 0, P(w_q), D, 1, P(dfull) + 4 * M * N * D, D, accumulate=True)
        hip.colsum(P(dkv), 2 * D, rows, 2 * D, P(sums2) + 8 * D, accumulate=False)
        hip.colsum(P(dq), D, cur, D, P(sums2) + 16 * D, accumulate=False)

    k_fwd(), k_bwd(), p_fwd(), p_bwd()
    torch.cuda.synchronize()
    tdx = t_bwd()[0]
    rec = dict(max_abs_kv_diff=float((kv - ref[0].detach()).abs().max()), max_abs_q_diff=float((q - ref[1].detach()).abs().max()),
               max_abs_dx_diff=float((dx - tdx).abs().max()), max_abs_pieces_kv_diff=float((kv2 - kv).abs().max()),
               max_abs_pieces_dx_diff=float((dfull.view(Fs, N, D)[M:] - dx).abs().max()))
    rec.update(timed({"kernel_fwd": k_fwd, "torch_fwd": lambda: t_fwd()[0].detach(), "pieces_fwd": p_fwd, "kernel_bwd": k_bwd,
                      "torch_bwd": t_bwd, "pieces_bwd": p_bwd}))
    # [*, D] float32 blocks moved once: forward mem, x, kv (2), q, x1; backward dkv (2), dq, mem, x, dx
    blocks = dict(fwd=(M + C + 2 * Fs + C + Fs) * N, bwd=(2 * Fs + C + M + C + C) * N)
    for d in ("fwd", "bwd"):
        med = rec[f"kernel_{d}"]["median_us"]
        rec[f"{d}_byte_floor_us"] = blocks[d] * D * 4 / HBM_BYTES_PER_S * 1e6
        rec[f"{d}_flop_floor_us"] = (4.0 * Fs + 2.0 * C) * N * D * D / F32_MATRIX_FLOPS * 1e6
        rec[f"{d}_fraction_of_byte_floor"] = rec[f"{d}_byte_floor_us"] / med
        rec[f"{d}_fraction_of_flop_floor"] = rec[f"{d}_flop_floor_us"] / med
        rec[f"{d}_torch_over_kernel"] = rec[f"torch_{d}"]["median_us"] / med
        rec[f"{d}_pieces_over_kernel"] = rec[f"pieces_{d}"]["median_us"] / med
    print(json.dumps({"shape": [D, M, C, N], **rec}), flush=True)
    return rec


if __name__ == "__main__":
    assert torch.cuda.is_available()
    res = {"-".join(map(str, sh)): case(*sh) for sh in SHAPES}
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)
