"""Transformer-XL's relative attention on the GPU (csrc/attn_xl.hip through hip.attn_xl_fwd / hip.attn_xl_bwd) against the plain
restatement tests/attn_xl_ref.py, which tests/test_attn_xl_reference.py holds to the real reference.

Bound, per tensor (this kernel family's rule, tests/test_gpu_rnn.py BOUNDS["step"]): max|got - ref64| <= 4 max|ref32 - ref64| +
1e-7 max|ref64|, ref32 / ref64 the restatement in float32 / float64 on the CPU: the kernel does the same float32 work in another
summation order.  On an MI355X the largest error / bound over all cases and tensors was 0.56 (dq); at C = 1, M = 0 the softmax is
over one key, every gradient but dval is exactly zero and so is its bound.  Every buffer is NaN-filled, has a leading dimension wider than its payload (k and val are the two halves of ONE
buffer, as an attention_kv product leaves them) and sentinel rows behind its last row."""
import pytest
import torch

from attn_xl_ref import NAMES, attn_xl_grads
from srl_amd import hip

DEV, A_F32, B_ABS = "cuda:0", 4.0, 1e-7
SENTINEL, PAD, EXTRA = -7.25, 3, 8   # sentinel rows behind each buffer; columns beyond the payload
# (nh, dh, C, M, N): the smallest launch; a rollout step over memory; pure causal; ragged in every dimension; across a 32-row tile
# and F = 64; wide heads; the largest C and F; N = None: three more batch rows than one head has slabs (from the workspace the
# library asks for), so that dr, du, dv fold over every slab and some workgroups walk two batch rows
CASES = [(1, 16, 1, 0, 1), (4, 16, 1, 3, 2), (4, 16, 5, 0, 3), (4, 16, 7, 5, 3), (4, 32, 33, 31, 2), (2, 64, 16, 48, 5),
         (4, 64, 64, 128, 1), (4, 16, 7, 5, None)]


def slabs_plus(nh, dh, C, M, more):
    per_slab = nh * (C + M + 2) * dh * 4
    return hip.attn_xl_bwd_workspace(nh, dh, C, M, 1 << 20) // per_slab + more


def make_inputs(nh, dh, C, M, N):
    g = torch.Generator().manual_seed(7 + 1000 * C + 10 * M + N + nh * dh)
    rn = lambda *s: torch.randn(*s, generator=g)
    F, W, s = C + M, nh * dh, dh ** -0.25   # q, k, r scaled so that the scores are O(1)
    return dict(q=s * rn(C, N, W), k=s * rn(F, N, W), val=rn(F, N, W), r=s * rn(F, W), u=0.5 * s * rn(nh, dh), v=0.5 * s * rn(nh, dh)), rn(C, N, W)


def padded(rows, width, src=None, ld=None):
    """[rows + PAD, ld] on the device: ``src`` (or NaN) in the payload columns, NaN beyond them, SENTINEL in the last PAD rows."""
    x = torch.full((rows + PAD, ld or width + EXTRA), float("nan"))
    if src is not None:
        x[:rows, :width] = src.reshape(rows, width)
    x[rows:] = SENTINEL
    return x.to(DEV)


def run(shape, inp, g, twice=False):
    nh, dh, C, M, N = shape
    F, W = C + M, nh * dh
    kv = padded(F * N, 2 * W)
    kv[:F * N, :W], kv[:F * N, W:2 * W] = inp["k"].reshape(F * N, W).to(DEV), inp["val"].reshape(F * N, W).to(DEV)
    b = dict(q=padded(C * N, W, inp["q"]), kv=kv, r=padded(F, W, inp["r"]), u=padded(1, W, inp["u"], W), v=padded(1, W, inp["v"], W),
             g=padded(C * N, W, g), out=padded(C * N, W), lse=padded(1, N * nh * C, ld=N * nh * C), dq=padded(C * N, W),
             dkv=padded(F * N, 2 * W), dr=padded(F, W), du=padded(1, W, ld=W), dv=padded(1, W, ld=W))
    ws = torch.full((hip.attn_xl_bwd_workspace(*shape) // 4,), float("nan"), device=DEV)   # (need not be cleared)
    p = {n: x.data_ptr() for n, x in b.items()}
    ld, ldkv = W + EXTRA, 2 * W + EXTRA
    hip.attn_xl_fwd(p["q"], ld, p["kv"], p["kv"] + 4 * W, ldkv, p["r"], ld, p["u"], p["v"], N, nh, dh, C, M, p["out"], ld, p["lse"])
    runs = []
    for _ in range(2 if twice else 1):
        hip.attn_xl_bwd(p["g"], ld, p["q"], ld, p["kv"], p["kv"] + 4 * W, ldkv, p["r"], ld, p["u"], p["v"], p["lse"], N, nh, dh, C, M,
                        p["dq"], ld, p["dkv"], p["dkv"] + 4 * W, ldkv, p["dr"], ld, p["du"], p["dv"], ws.data_ptr(), ws.numel() * 4)
        torch.cuda.synchronize()
        runs.append({n: b[n][:rows, :W].cpu() for n, rows in (("dr", F), ("du", 1), ("dv", 1))})
    c = {n: x.cpu() for n, x in b.items()}
    for n, x in c.items():
        assert bool((x[-PAD:] == SENTINEL).all()), (n, "rows behind the last row were written")
    for n, rows, width in (("out", C * N, W), ("dq", C * N, W), ("dkv", F * N, 2 * W), ("dr", F, W)):
        assert bool(torch.isnan(c[n][:rows, width:]).all()), (n, "columns beyond the payload were written")
    got = dict(out=c["out"][:C * N, :W], dq=c["dq"][:C * N, :W], dk=c["dkv"][:F * N, :W], dval=c["dkv"][:F * N, W:2 * W],
               dr=c["dr"][:F, :W], du=c["du"][:1], dv=c["dv"][:1], lse=c["lse"][:1])
    return got, runs


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_attn_xl_vs_float64(case):
    shape = case[:4] + (case[4] or slabs_plus(*case[:4], 3),)
    inp, g = make_inputs(*shape)
    r64, r32 = (attn_xl_grads(inp, g, dt) for dt in (torch.float64, torch.float32))
    got, runs = run(shape, inp, g, twice=case[4] is None)
    rows = []
    for name, want in r64.items():
        v = got[name].reshape(want.shape)
        assert bool(torch.isfinite(v).all()), (name, "an element not written, or not finite")
        err = float((v.double() - want).abs().max())
        rows.append((name, err, A_F32 * float((r32[name] - want).abs().max()) + B_ABS * float(want.abs().max())))
    print(f"\nattn_xl {shape}: (tensor, error, bound)", *rows, sep="\n  ")
    assert bool(torch.isfinite(got["lse"]).all())
    for name, err, lim in rows:
        assert err <= lim, (name, err, lim)
    for name in runs[0] if len(runs) == 2 else ():
        assert torch.equal(runs[0][name], runs[1][name]), (name, "two backward runs on the same inputs differ")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 8, 4, 4, 2), (4, 16, 1, 192, 2), (4, 16, 65, 0, 2)], ids=str)
def test_unsupported_sizes_raise_and_launch_nothing(shape):
    nh, dh, C, M, N = shape
    W, ld = nh * dh, nh * dh + EXTRA
    x, kv, out = padded(C * N, W), padded((C + M) * N, 2 * W), padded(C * N, W)
    lse, uv = padded(1, N * nh * C, ld=N * nh * C), padded(1, W, torch.ones(W), W)
    with pytest.raises(hip.HipError):
        hip.attn_xl_fwd(x.data_ptr(), ld, kv.data_ptr(), kv.data_ptr() + 4 * W, 2 * W + EXTRA, kv.data_ptr(), 2 * W + EXTRA,
                        uv.data_ptr(), uv.data_ptr(), N, nh, dh, C, M, out.data_ptr(), ld, lse.data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:C * N]).all()) and bool(torch.isnan(lse[:1]).all())
