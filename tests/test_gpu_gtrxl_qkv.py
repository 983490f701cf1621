"""The front of a GTrXL layer on the GPU (csrc/gtrxl_qkv.hip through hip.gtrxl_qkv_fwd / _bwd / _wgrad) against the plain restatement
tests/gtrxl_qkv_ref.py, which tests/test_gtrxl_qkv_reference.py holds to the real reference.

Bound, per tensor (this kernel family's rule, tests/test_gpu_gtrxl_gate.py): max|got - ref64| <= 4 max|ref32 - ref64| + 1e-7 max|ref64|,
ref32 / ref64 the restatement in float32 / float64 on the CPU.  dw_kv and dw_q come out of srl_gemm: where srl_gemm_family says a
product takes another family than float32 MFMA they are held, element by element, to that family's rule: |got - float64 product of
the operands srl_gemm was given| <= 2e-6 sum_k |a| |b|.  On an MI355X the largest error / bound over all cases and tensors was 0.85
(db_kv at D = 256, 8 281 rows; q 0.72 at D = 64, one row; kv 0.37, dx 0.26).  Every buffer is NaN-filled, has a leading dimension wider than its payload
and sentinel rows behind its last row; the workspace is NaN-filled; gamma holds one exact zero."""
import pytest
import torch

from gtrxl_qkv_ref import gtrxl_qkv
from srl_amd import hip

DEV, A_F32, B_ABS, X3_REL = "cuda:0", 4.0, 1e-7, 2e-6
SENTINEL, PAD, EXTRA = -7.25, 3, 8   # sentinel rows behind each buffer; columns beyond the payload
SUMS, TILE = ("dgamma", "dbeta", "db_kv", "db_q"), {64: 128, 128: 64, 256: 32}   # TILE: the row tile, 8192 / D (srl_hip.h)
# (D, M, C, N, keep): no memory, one row; the seam inside a ragged first tile; the seam one row into the second tile at 256 and at 128;
# keep = NULL; a rollout step; N = None: F = 7 and three more tiles than workgroups (from the workspace the library asks for), so that
# some workgroups walk two tiles and the sums fold over every slab -- the backward run twice, bits compared
CASES = [(64, 0, 1, 1, True), (64, 3, 2, 5, True), (256, 1, 1, 33, True), (128, 2, 1, 33, True), (128, 4, 3, 17, False),
         (256, 64, 1, 2, True), (64, 5, 2, None, True), (128, 5, 2, None, True), (256, 5, 2, None, True)]
OUT = dict(kv=2, kv0=2, q=1, q0=1, x1=1, dx=1)   # row buffers the launches write: payload width in units of D


def make_inputs(D, M, C, N, keep):
    g = torch.Generator().manual_seed(13 + D + M + C + N)
    rn = lambda *s: torch.randn(*s, generator=g)
    inp = dict(mem=rn(M, N, D), x=rn(C, N, D), gamma=1 + 0.3 * rn(D), beta=0.3 * rn(D), w_kv=D ** -0.5 * rn(2 * D, D), b_kv=0.1 * rn(2 * D),
               w_q=D ** -0.5 * rn(D, D), b_q=0.1 * rn(D))
    inp["gamma"][3] = 0.0
    if keep:
        inp["keep"] = torch.ones(N)
        inp["keep"][0], inp["keep"][-1] = 0.0, 0.5   # (N = 1: 0.5)
    return inp, rn(M + C, N, 2 * D), rn(C, N, D)


def padded(rows, width, src=None, ld=None):
    """[rows + PAD, ld] on the device: ``src`` (or NaN) in the payload columns, NaN beyond them, SENTINEL in the last PAD rows."""
    x = torch.full((rows + PAD, ld or width + EXTRA), float("nan"))
    if src is not None:
        x[:rows, :width] = src.reshape(rows, width)
    x[rows:] = SENTINEL
    return x.to(DEV)


def run(D, M, C, N, inp, dkv, dq, twice):
    F, ld, ld2 = M + C, D + EXTRA, 2 * D + EXTRA
    nrows = {n: (F if n in ("kv", "kv0", "x1") else C) * N for n in OUT}
    b = dict(mem=padded(M * N, D, inp["mem"]), x=padded(C * N, D, inp["x"]), dkv=padded(F * N, 2 * D, dkv), dq=padded(C * N, D, dq),
             kv=padded(F * N, 2 * D), kv0=padded(F * N, 2 * D), q=padded(C * N, D), q0=padded(C * N, D), x1=padded(F * N, D),
             dx=padded(C * N, D), stats=padded(F * N, 2, ld=2), dw_kv=padded(2 * D, D, ld=D), dw_q=padded(D, D, ld=D))
    for n in ("gamma", "beta", "b_kv", "b_q", "keep") + SUMS:
        w = 2 * D if "b_kv" in n else N if n == "keep" else D
        b[n] = padded(1, w, inp.get(n), w + (-w) % 4)
    b["w_kv"], b["w_q"] = padded(2 * D, D, inp["w_kv"], D), padded(D, D, inp["w_q"], D)
    ws = torch.full((hip.gtrxl_qkv_bwd_workspace(D, F * N) // 4,), float("nan"), device=DEV)   # (need not be cleared)
    p = {n: x.data_ptr() for n, x in b.items()}
    keep = p["keep"] if "keep" in inp else None
    fwd = lambda kv, q, *save: hip.gtrxl_qkv_fwd(p["mem"], ld, p["x"], ld, keep, p["gamma"], p["beta"], p["w_kv"], p["b_kv"], p["w_q"],
                                                 p["b_q"], M, C, N, D, kv, ld2, q, ld, *save)
    fwd(p["kv0"], p["q0"])   # a rollout: nothing saved
    fwd(p["kv"], p["q"], p["x1"], ld, p["stats"])
    runs = []
    for _ in range(2 if twice else 1):
        hip.gtrxl_qkv_bwd(p["dkv"], ld2, p["dq"], ld, p["mem"], ld, p["x"], ld, keep, p["stats"], p["gamma"], p["w_kv"], p["w_q"], M, C, N, D,
                          p["dx"], ld, p["dgamma"], p["dbeta"], p["db_kv"], p["db_q"], ws.data_ptr(), ws.numel() * 4)
        torch.cuda.synchronize()
        runs.append({n: (b[n][:C * N, :D] if n == "dx" else b[n][0]).cpu() for n in SUMS + ("dx",)})
    split = max(1, C * N // 512)   # the trainers' rule for a long row count (hipnet._split_for): slices of at least 512 rows
    wsk = torch.full((split * 2 * D * D,), float("nan"), device=DEV)
    hip.gtrxl_qkv_wgrad(p["dkv"], ld2, p["x1"], ld, p["dq"], ld, p["x"], ld, M, C, N, D, p["dw_kv"], p["dw_q"], split_k=split,
                        workspace=wsk.data_ptr() if split > 1 else None)
    torch.cuda.synchronize()
    c = {n: x.cpu() for n, x in b.items()}
    for n, x in c.items():
        assert bool((x[-PAD:] == SENTINEL).all()), (n, "rows behind the last row were written")
    for n, r in nrows.items():
        assert bool(torch.isnan(c[n][:r, OUT[n] * D:]).all()), (n, "columns beyond the payload were written")
    got = {n: c[n][:r, :OUT[n] * D] for n, r in nrows.items()}
    assert torch.equal(got["kv"], got["kv0"]) and torch.equal(got["q"], got["q0"]), "kv or q differs between x1 = stats = NULL and the saving run"
    got.update(stats=c["stats"][:F * N], dw_kv=c["dw_kv"][:2 * D], dw_q=c["dw_q"][:D], **{n: c[n][0] for n in SUMS})
    return got, runs, p


def wgrad_other_family(name, D, M, C, N, got, inp, dkv, dq, p):
    """None where ``name``'s product takes the float32 MFMA family; else (float64 product of the operands GIVEN, its elements' bounds)."""
    rows, W, A, B = ((M + C) * N, 2 * D, p["dkv"], p["x1"]) if name == "dw_kv" else (C * N, D, p["dq"], p["x"])
    if hip.gemm_family(W, D, rows, A, W + EXTRA, B, D + EXTRA, None, None, a_kmajor=True, b_kmajor=True) == hip.FAMILY_F32:
        return None
    a, bm = (dkv, got["x1"]) if name == "dw_kv" else (dq, inp["x"])
    a, bm = a.reshape(rows, W).double(), bm.reshape(rows, D).double()
    return a.T @ bm, X3_REL * (a.abs().T @ bm.abs())


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_gtrxl_qkv_vs_float64(case):
    D, M, C, N, keep = case
    N = N or ((hip.gtrxl_qkv_bwd_workspace(D, 1 << 30) // (20 * D) + 3) * TILE[D] - 5) // (M + C)
    inp, dkv, dq = make_inputs(D, M, C, N, keep)
    r64, r32 = (gtrxl_qkv(inp, dkv, dq, dt) for dt in (torch.float64, torch.float32))
    got, runs, p = run(D, M, C, N, inp, dkv, dq, twice=case[3] is None)
    table = []
    for name, want in r64.items():
        v = got[name].reshape(want.shape)
        assert bool(torch.isfinite(v).all()), (name, "an element not written, or not finite")
        other = wgrad_other_family(name, D, M, C, N, got, inp, dkv, dq, p) if name.startswith("dw_") else None
        if other is None:
            err = float((v.double() - want).abs().max())
            lim = A_F32 * float((r32[name] - want).abs().max()) + B_ABS * float(want.abs().max())
        else:   # the largest error in units of its own element's bound
            err, lim = float(((v.double() - other[0]).abs() / other[1]).max()), 1.0
        table.append((name, err, lim))
    print(f"\ngtrxl_qkv D = {D}, M = {M}, C = {C}, N = {N}: (tensor, error, bound)", *table, sep="\n  ")
    assert not [t for t in table if t[1] > t[2]], [t for t in table if t[1] > t[2]]
    for name in runs[0] if len(runs) == 2 else ():
        assert torch.equal(runs[0][name], runs[1][name]), (name, "two runs on the same inputs differ")


@pytest.mark.gpu
@pytest.mark.parametrize("fault", ["D = 96", "ld < D", "workspace one byte short"])
def test_refusals_raise_and_launch_nothing(fault):
    D, M, C, N = (96 if fault == "D = 96" else 64), 1, 1, 3
    ld = D - 4 if fault == "ld < D" else D + EXTRA
    x, w, q, kv, dx = padded(N, D, torch.ones(N, D)), padded(2 * D, D, torch.ones(2 * D, D), D), padded(N, D), padded(2 * N, 2 * D), padded(N, D)
    sums, ws = padded(1, 5 * D, ld=5 * D), torch.empty(5 * 64 + 64, device=DEV)
    wsb = hip.gtrxl_qkv_bwd_workspace(64, 2 * N) - (fault == "workspace one byte short")
    X, W, S = x.data_ptr(), w.data_ptr(), sums.data_ptr()
    if fault != "workspace one byte short":
        with pytest.raises(hip.HipError):
            hip.gtrxl_qkv_fwd(X, D + EXTRA, X, D + EXTRA, None, W, W, W, W, W, W, M, C, N, D, kv.data_ptr(), 2 * D + EXTRA, q.data_ptr(), ld)
    with pytest.raises(hip.HipError):
        hip.gtrxl_qkv_bwd(kv.data_ptr(), 2 * D + EXTRA, X, D + EXTRA, X, D + EXTRA, X, D + EXTRA, None, W, W, W, W, M, C, N, D, dx.data_ptr(), ld,
                          S, S + 4 * D, S + 8 * D, S + 16 * D, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t[:-PAD]).all()) for t in (q, kv, dx, sums))
