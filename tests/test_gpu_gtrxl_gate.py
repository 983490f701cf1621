"""GTrXL's GRU-style gating unit on the GPU (csrc/gtrxl_gate.hip through hip.gtrxl_gate_fwd / _bwd / _wgrad) against the plain
restatement tests/gtrxl_gate_ref.py, which tests/test_gtrxl_gate_reference.py holds to the real reference.

Bound, per tensor (this kernel family's rule, tests/test_gpu_rnn.py BOUNDS["step"]): max|got - ref64| <= 4 max|ref32 - ref64| +
1e-7 max|ref64|, ref32 / ref64 the restatement in float32 / float64 on the CPU.  dw_y and dw_x come out of srl_gemm: where
srl_gemm_family says a product takes another family than float32 MFMA they are held, element by element, to what
tests/test_gpu_kernels.py::test_gemm_bf16x3_is_as_accurate_as_the_float32_mfma asks of that family: |got - float64 product of the
operands srl_gemm was given| <= 2e-6 sum_k |a| |b|.  On an MI355X the largest error / bound over all cases and tensors was 0.52
(gates at D = 64, rows = 1; dw_x 0.51 there).  Every buffer is NaN-filled, has a leading dimension wider than its payload and sentinel
rows behind its last row."""
import pytest
import torch

from gtrxl_gate_ref import gtrxl_gate
from srl_amd import hip

DEV, A_F32, B_ABS, X3_REL = "cuda:0", 4.0, 1e-7, 2e-6
SENTINEL, PAD, EXTRA = -7.25, 3, 8   # sentinel rows behind each buffer; columns beyond the payload
TILE = {64: 128, 128: 64, 256: 32}   # the row tile, 8192 / D (srl_hip.h)
# (D, rows): one row in a ragged tile; across a 32-row block; across the tile and ragged (tile + 1) at every width; two tiles and
# ragged at D = 256; rows = None: three more tiles than workgroups (from the workspace the library asks for), so that some
# workgroups walk two tiles and d_bg folds over every slab -- run twice, bits compared
CASES = [(64, 1), (64, 33), (64, 129), (128, 7), (128, 65), (256, 1), (256, 33), (256, 70), (128, None), (256, None), (64, None)]


def rows_for(D, rows):
    return rows or (hip.gtrxl_gate_bwd_workspace(D, 1 << 30) // (4 * D) + 3) * TILE[D] - 5


def make_inputs(D, rows):
    g = torch.Generator().manual_seed(11 + D + rows)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(x=rn(rows, D), y=rn(rows, D), w_y=D ** -0.5 * rn(3 * D, D), w_x=D ** -0.5 * rn(3 * D, D), bg=2 + 0.1 * rn(D)), rn(rows, D)


def padded(rows, width, src=None, ld=None):
    """[rows + PAD, ld] on the device: ``src`` (or NaN) in the payload columns, NaN beyond them, SENTINEL in the last PAD rows."""
    x = torch.full((rows + PAD, ld or width + EXTRA), float("nan"))
    if src is not None:
        x[:rows, :width] = src.reshape(rows, width)
    x[rows:] = SENTINEL
    return x.to(DEV)


def run(D, rows, inp, dg, twice):
    b = dict(x=padded(rows, D, inp["x"]), y=padded(rows, D, inp["y"]), dg=padded(rows, D, dg), w_y=padded(3 * D, D, inp["w_y"], D),
             w_x=padded(3 * D, D, inp["w_x"], D), bg=padded(1, D, inp["bg"], D), g=padded(rows, D), g0=padded(rows, D),
             gates=padded(rows, 3 * D), dx=padded(rows, D), dy=padded(rows, D), rx=padded(rows, D), d_bg=padded(1, D, ld=D),
             dw_y=padded(3 * D, D, ld=D), dw_x=padded(3 * D, D, ld=D))
    ws = torch.full((hip.gtrxl_gate_bwd_workspace(D, rows) // 4,), float("nan"), device=DEV)   # (need not be cleared)
    p = {n: x.data_ptr() for n, x in b.items()}
    ld, ldg = D + EXTRA, 3 * D + EXTRA
    hip.gtrxl_gate_fwd(p["x"], ld, p["y"], ld, p["w_y"], p["w_x"], p["bg"], rows, D, p["g0"], ld)   # a rollout: nothing saved
    runs = []
    for _ in range(2 if twice else 1):
        hip.gtrxl_gate_fwd(p["x"], ld, p["y"], ld, p["w_y"], p["w_x"], p["bg"], rows, D, p["g"], ld, p["gates"], ldg)
        torch.cuda.synchronize()
        gates = b["gates"][:rows, :3 * D].cpu()
        hip.gtrxl_gate_bwd(p["dg"], ld, p["x"], ld, p["y"], ld, p["w_y"], p["w_x"], p["gates"], ldg, rows, D, p["dx"], ld, p["dy"], ld,
                           p["rx"], ld, p["d_bg"], ws.data_ptr(), ws.numel() * 4)
        torch.cuda.synchronize()
        runs.append({n: b[n][:r, :D].cpu() for n, r in (("d_bg", 1), ("dx", rows), ("dy", rows))})
    hip.gtrxl_gate_wgrad(p["gates"], ldg, p["x"], ld, p["y"], ld, p["rx"], ld, rows, D, p["dw_y"], p["dw_x"])
    torch.cuda.synchronize()
    c = {n: x.cpu() for n, x in b.items()}
    for n, x in c.items():
        assert bool((x[-PAD:] == SENTINEL).all()), (n, "rows behind the last row were written")
    for n, width in (("g", D), ("g0", D), ("gates", 3 * D), ("dx", D), ("dy", D), ("rx", D)):
        assert bool(torch.isnan(c[n][:rows, width:]).all()), (n, "columns beyond the payload were written")
    assert torch.equal(c["g"][:rows, :D], c["g0"][:rows, :D]), "g differs between gates = NULL and the run that saves them"
    got = dict(g=c["g"][:rows, :D], gates=gates, dx=c["dx"][:rows, :D], dy=c["dy"][:rows, :D], A=c["gates"][:rows, :3 * D],
               rx=c["rx"][:rows, :D], d_bg=c["d_bg"][0], dw_y=c["dw_y"][:3 * D], dw_x=c["dw_x"][:3 * D])
    return got, runs, p


def wgrad_other_family(name, D, rows, got, inp, p):
    """None where every product behind ``name`` takes the float32 MFMA family; else (the float64 product of the operands srl_gemm
    was GIVEN -- the kernel's own A and rx, themselves held by the 4 x rule --, 2e-6 sum_k |a| |b| per element)."""
    ld, ldg, D2 = D + EXTRA, 3 * D + EXTRA, 2 * D
    calls = [(3 * D, p["gates"], p["y"])] if name == "dw_y" else [(D2, p["gates"], p["x"]), (D, p["gates"] + 8 * D, p["rx"])]
    if all(hip.gemm_family(M, D, rows, A, ldg, B, ld, None, None, a_kmajor=True, b_kmajor=True) == hip.FAMILY_F32 for M, A, B in calls):
        return None
    A, x, y, rx = got["A"].double(), inp["x"].double(), inp["y"].double(), got["rx"].double()
    if name == "dw_y":
        return A.T @ y, X3_REL * (A.abs().T @ y.abs())
    return (torch.cat([A[:, :D2].T @ x, A[:, D2:].T @ rx]),
            X3_REL * torch.cat([A[:, :D2].abs().T @ x.abs(), A[:, D2:].abs().T @ rx.abs()]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_gtrxl_gate_vs_float64(case):
    D, rows = case[0], rows_for(*case)
    inp, dg = make_inputs(D, rows)
    r64, r32 = (gtrxl_gate(inp, dg, dt) for dt in (torch.float64, torch.float32))
    got, runs, p = run(D, rows, inp, dg, twice=case[1] is None)
    table = []
    for name in ("g", "gates", "dx", "dy", "A", "rx", "d_bg", "dw_y", "dw_x"):
        want, v = r64[name], got[name].reshape(r64[name].shape)
        assert bool(torch.isfinite(v).all()), (name, "an element not written, or not finite")
        other = wgrad_other_family(name, D, rows, got, inp, p) if name.startswith("dw_") else None
        if other is None:
            err = float((v.double() - want).abs().max())
            lim = A_F32 * float((r32[name] - want).abs().max()) + B_ABS * float(want.abs().max())
        else:   # the largest error in units of its own element's bound
            err, lim = float(((v.double() - other[0]).abs() / other[1]).max()), 1.0
        table.append((name, err, lim))
    print(f"\ngtrxl_gate D = {D}, rows = {rows}: (tensor, error, bound)", *table, sep="\n  ")
    assert not [t for t in table if t[1] > t[2]], [t for t in table if t[1] > t[2]]
    for name in runs[0] if len(runs) == 2 else ():
        assert torch.equal(runs[0][name], runs[1][name]), (name, "two runs on the same inputs differ")


@pytest.mark.gpu
@pytest.mark.parametrize("fault", ["D = 96", "ld < D", "workspace one byte short"])
def test_refusals_raise_and_launch_nothing(fault):
    D, rows = (96 if fault == "D = 96" else 64), 5
    ld = D - 4 if fault == "ld < D" else D + EXTRA
    x, w, out, gates = padded(rows, D, torch.ones(rows, D)), padded(3 * D, D, torch.ones(3 * D, D), D), padded(rows, D), padded(rows, 3 * D)
    d_bg, ws = padded(1, D, ld=D), torch.empty(64, device=DEV)
    wsb = hip.gtrxl_gate_bwd_workspace(64, rows) - (fault == "workspace one byte short")
    if fault != "workspace one byte short":
        with pytest.raises(hip.HipError):
            hip.gtrxl_gate_fwd(x.data_ptr(), ld, x.data_ptr(), ld, w.data_ptr(), w.data_ptr(), w.data_ptr(), rows, D, out.data_ptr(), ld,
                               gates.data_ptr(), 3 * D + EXTRA)
    with pytest.raises(hip.HipError):
        hip.gtrxl_gate_bwd(x.data_ptr(), D + EXTRA, x.data_ptr(), D + EXTRA, x.data_ptr(), D + EXTRA, w.data_ptr(), w.data_ptr(),
                           gates.data_ptr(), 3 * D + EXTRA, rows, D, out.data_ptr(), ld, out.data_ptr(), D + EXTRA, None, 0,
                           d_bg.data_ptr(), ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t[:-PAD]).all()) for t in (out, gates, d_bg))
