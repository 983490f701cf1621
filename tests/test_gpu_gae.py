"""`srl_gae_scan` (csrc/gae.hip) held to the float64 statement tests/gae_ref.py on every branch of its launch choice and at every
seam of its tilings.  The cases, their inputs and what each is for: tests/gae_cases.py; that the reference, the bound and the cases
can fail: tests/test_gae_reference.py.

Per element, nothing exempt:   |adv_gpu - g| <= 2^-24 |g| + 4 T 2^-53 A   (gae_ref.bound; one float32 rounding + the float64
rounding of both evaluations; nothing in it is measured);  ret_gpu is float32(adv_gpu) + v', one float32 add, bit for bit;
stats[0] is the mask count exactly, stats[1] / stats[2] are the float64 sums of the GPU's own adv to 2 N 2^-53 sum|x| / sum x^2."""
import numpy as np
import pytest
import torch

import gae_cases as gc
import gae_ref
from srl_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 7.0
GUARD = 4   # elements behind the pad row T


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def shifted(x, align, off):
    """`x` on the device in a flat buffer one element longer, viewed from element 1: `off` bytes past an `align`-byte boundary."""
    flat = torch.empty(x.size + 1, dtype=torch.as_tensor(x[:0]).dtype, device=DEV)
    flat[1:] = dev(x).reshape(-1)
    out = flat[1:].view(*x.shape)
    assert out.data_ptr() % align == off and out.is_contiguous()
    return out


def out_buffers(T, B, Nc):
    """adv, ret [T + 1, B, Nc] inside flat buffers GUARD elements longer, all at FILL."""
    n = (T + 1) * B * Nc
    flat = [torch.full((n + GUARD,), FILL, device=DEV) for _ in range(2)]
    return flat, [f[:n].view(T + 1, B, Nc) for f in flat]


def check_stats(stats, adv, on_reset, N):
    """The three sums against a float64 recomputation from the GPU's own adv."""
    s = gae_ref.stats(adv, on_reset)
    assert stats[0] == s["n"]
    assert abs(stats[1] - s["s"]) <= 2 * N * gae_ref.U64 * s["sabs"], (stats[1], s)
    assert abs(stats[2] - s["q"]) <= 2 * N * gae_ref.U64 * s["q"], (stats[2], s)


def ticket(ws):
    return int(ws.view(torch.int32)[0].item())


def partial_sums(ws, grid):
    """[grid, 3]: what the workgroups left in a workspace (8 bytes of ticket, then three doubles per workgroup)."""
    return ws.view(torch.float64)[1:1 + 3 * grid].view(grid, 3)


@pytest.mark.parametrize("name", [c.name for c in gc.CASES])
def test_gae_case(name):
    case = gc.BY_NAME[name]
    plan = gc.plan_of(case)
    gc.assert_on_branch(case, plan)
    a = gc.build(case, plan)
    gc.check_inputs(case, a)
    T, B, Nc = case.T, case.B, case.Nc
    N = T * B * Nc
    r = gc.reference(a)
    g, bnd = r["g"], gae_ref.bound(r["g"], r["A"], T)

    value = shifted(a["value"], 16, 4) if case.misalign == "value" else dev(a["value"])
    done = shifted(a["done"], 4, 1) if case.misalign == "done" else dev(a["done"])
    tens = lambda x: dev(x) if isinstance(x, np.ndarray) else x
    args = [dev(a["reward"]), value, done, dev(a["truncated"]), dev(a["on_reset"]), tens(a["gamma"]), tens(a["lmbda"])]
    kw = dict(imp_ratio=None if a["ratio"] is None else dev(a["ratio"]), rho=a["rho"], c=a["c"])
    ws = hip.gae_scan_workspace(B, Nc, DEV)

    def launch(workspace):
        flat, (adv, ret) = out_buffers(T, B, Nc)
        assert adv.data_ptr() % 16 == 0 and ret.data_ptr() % 16 == 0
        stats = torch.full((3,), 123.0, dtype=torch.float64, device=DEV)   # overwritten, not accumulated
        hip.gae_scan(*args, adv, ret, stats=stats, workspace=workspace, **kw)
        torch.cuda.synchronize()
        for f in flat:   # the pad row T and what lies behind the last column are the caller's
            assert (f[N:] == FILL).all()
        adv, stats = adv.cpu().numpy()[:T], stats.cpu().numpy()
        check_stats(stats, adv, a["on_reset"], N)
        return adv, ret.cpu().numpy()[:T], stats

    adv, ret, _ = launch(None)
    err = np.abs(adv.astype(np.float64) - g)
    worst = float((err[bnd > 0] / bnd[bnd > 0]).max())
    print(f"{name}: worst error / bound = {worst:.3f}")
    assert (err <= bnd).all(), (name, worst)
    assert np.array_equal(ret, adv + r["v"][:T]), name
    adv1, ret1, stats1 = launch(ws)
    adv2, ret2, stats2 = launch(ws)
    for x, y in ((adv1, adv), (adv2, adv), (ret1, ret), (ret2, ret)):
        assert np.array_equal(x, y)
    assert ticket(ws) == 0   # back at zero for the next launch
    if plan["workspace"]:   # partial sums, added in workgroup order: the same bits from launch to launch
        assert np.array_equal(stats1, stats2)
        assert float(partial_sums(ws, plan["grid"])[:, 0].sum().item()) == stats1[0]
    else:                   # ignored: it stays as the caller zeroed it
        assert (ws == 0).all()


@pytest.mark.parametrize("T,B", [(5, 0), (0, 8), (0, 0)])
def test_gae_empty_batches_leave_zero_stats(T, B):
    z = lambda dt: torch.zeros((T + 1, B, 1), dtype=dt, device=DEV)
    for workspace in (None, hip.gae_scan_workspace(B, 1, DEV)):
        stats = torch.full((3,), 123.0, dtype=torch.float64, device=DEV)
        adv, ret = torch.full((T + 1, B, 1), FILL, device=DEV), torch.full((T + 1, B, 1), FILL, device=DEV)
        hip.gae_scan(z(torch.float32), z(torch.float32), z(torch.uint8), z(torch.uint8), z(torch.uint8), 0.99, 0.97, adv, ret,
                     stats=stats, workspace=workspace)
        assert (stats.cpu().numpy() == 0).all() and (adv == FILL).all() and (ret == FILL).all()


@pytest.mark.parametrize("B,honoured", [(98304, 0), (98300, 1)])
def test_gae_workspace_cutoff(B, honoured):
    """From 98 304 columns on a workspace is ignored (memset + atomics: it stays as the caller zeroed it) and stats are still
    overwritten, not accumulated; below, the workgroups leave their partial sums in it."""
    T = 4
    plan = hip.gae_scan_plan(T, B)
    assert plan["workspace"] == honoured and plan["kernel"] == gc.REG
    a = gc.build(gc.Case(f"cutoff_B{B}", gc.REG, plan["width"], plan["L"], False, T, B), plan)
    args = [dev(a[k]) for k in ("reward", "value", "done", "truncated", "on_reset")]
    ws = hip.gae_scan_workspace(B, 1, DEV)
    out = []
    for _ in range(2):
        _, (adv, ret) = out_buffers(T, B, 1)
        stats = torch.full((3,), 123.0, dtype=torch.float64, device=DEV)
        hip.gae_scan(*args, 0.99, 0.97, adv, ret, stats=stats, workspace=ws)
        torch.cuda.synchronize()
        out.append(stats.cpu().numpy())
        check_stats(out[-1], adv.cpu().numpy()[:T], a["on_reset"], T * B)
    assert ticket(ws) == 0
    if honoured:
        assert np.array_equal(out[0], out[1]) and float(partial_sums(ws, plan["grid"])[:, 0].sum().item()) == out[0][0]
    else:
        assert (ws == 0).all()
