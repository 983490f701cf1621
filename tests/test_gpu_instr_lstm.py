"""The fused instruction encoder (csrc/instr_lstm.hip) beyond a workgroup's first tile: seeded cases with enough rows that every
workgroup of the persistent grid takes a second tile, one a third, and the last tile is ragged; a backward through one workgroup's
workspace slab; the longest sequence -- against the float64 restatement (tests/instr_lstm_ref.py), every element, by the project's
rule: an error of at most 3 x the float32 statement's own error plus 2e-6 of the tensor's largest float64 element, per tensor.

Tokens, ``d_out`` and ``out`` have padded pitches and 8 guard rows behind the rows the kernel is told about (NaN where it must not
read, 7.0 where it must not write); the gradient buffers start at 0.5 and take two backward calls."""
import functools

import numpy as np
import pytest
import torch

import instr_lstm_ref as ref
import srl_amd
from dmlab_cases import BLOCK_PARAMS
from srl_amd import hip
from test_gpu_dmlab import bound64

srl_amd.register_all()
pytestmark = pytest.mark.gpu

PAD, GUARD, TILE = 3, 8, 32


def case_rows(case):
    """many tiles: two full rounds of the grid, one more tile and a ragged rest, from the library's own grid; else the issue's."""
    V, Ed, H, L = ref.CASES[case]
    if case.startswith("many_tiles"):
        G = hip.instr_lstm_groups(hip.instr_lstm_desc(V, Ed, H, L), 1 << 24)   # (so many rows that the grid is at its cap)
        return 2 * TILE * G + TILE + 5
    return 70 if case == "longest" else 101


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's data and the float32 / float64 statements of it, computed once."""
    c = ref.draw_case(case, case_rows(case), seed=40 + list(ref.CASES).index(case))
    return c, ref.encoder(c["params"], c["tok"], c["cot"], torch.float32), ref.encoder(c["params"], c["tok"], c["cot"], torch.float64)


def padded(a, fill):
    """[n, w] -> device [n + GUARD, w + PAD] holding ``fill`` around the array."""
    n, w = a.shape
    t = torch.full((n + GUARD, w + PAD), fill, dtype=torch.float32)
    t[:n, :w] = torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda()


class Device:
    """A drawn case on the device: parameters, gradient buffers at 0.5, the descriptor, padded tokens and cotangent."""

    def __init__(self, c):
        self.H, self.L, self.rows = c["H"], c["L"], c["tok"].shape[0]
        self.params = {k: torch.from_numpy(v).cuda() for k, v in c["params"].items()}
        self.grads = {k: torch.full_like(v, 0.5) for k, v in self.params.items()}
        self.desc = hip.instr_lstm_desc(c["V"], c["Ed"], c["H"], c["L"], {f: self.params[k].data_ptr() for f, k in BLOCK_PARAMS.items()},
                                        {f: self.grads[k].data_ptr() for f, k in BLOCK_PARAMS.items()})
        self.tok, self.cot = padded(c["tok"], np.nan), padded(c["cot"], np.nan)
        self.slab = 2 * self.L * self.H * TILE * 4   # one workgroup's states, bytes

    def fwd(self, rows=None):
        out = torch.full((self.rows + GUARD, self.H + PAD), 7.0, dtype=torch.float32, device="cuda")
        hip.instr_lstm_fwd(self.desc, self.tok.data_ptr(), self.L + PAD, False, self.rows if rows is None else rows, out.data_ptr(), self.H + PAD)
        return out.cpu().numpy()

    def bwd(self, ws_bytes, rows=None):
        ws = torch.empty(max(ws_bytes, 4) // 4 + 1, dtype=torch.float32, device="cuda")
        hip.instr_lstm_bwd(self.desc, self.tok.data_ptr(), self.L + PAD, False, self.rows if rows is None else rows, self.cot.data_ptr(),
                           self.H + PAD, ws.data_ptr(), ws_bytes)
        torch.cuda.synchronize()


def check_grads(tag, dev, call, g32, g64):
    worst = 0.0
    for k, t in dev.grads.items():
        err, bound = np.abs(t.cpu().numpy().astype(np.float64) - 0.5 - call * g64[k]).max(), call * bound64(g32[k], g64[k])
        worst = max(worst, err / bound)
        print(f"{tag} call {call} {k}: error {err:.3e} bound {bound:.3e}")
        assert err <= bound, (k, call, err, bound)
    assert (dev.grads[ref.EMB][0] == 0.5).all()   # row 0 of the table's gradient: exactly as it was
    return worst


@pytest.mark.parametrize("case", ref.CASES)
def test_case_vs_float64(case):
    c, (out32, g32), (out64, g64) = reference(case)
    dev = Device(c)
    rows, H = dev.rows, dev.H
    assert hip.instr_lstm_supported(c["V"], c["Ed"], H, c["L"])
    tiles = -(-rows // TILE)
    full = hip.instr_lstm_bwd_workspace(dev.desc, rows)
    gf, gb = hip.instr_lstm_groups(dev.desc, rows), hip.instr_lstm_groups(dev.desc, rows, full)
    print(f"\n{case}: rows {rows}, tiles {tiles}, forward groups {gf}, backward groups {gb} on {full} bytes of workspace")
    assert gf == gb >= 1 and full == gb * dev.slab
    if case.startswith("many_tiles"):   # every workgroup takes a second tile, one takes a third, and the last tile is ragged
        assert tiles >= 2 * gf + 1 and rows % TILE != 0

    got = dev.fwd()
    assert (got[:rows, H:] == 7.0).all() and (got[rows:] == 7.0).all()   # pad columns and guard rows stay
    err, bound = np.abs(got[:rows, :H] - out64).max(), bound64(out32, out64)
    worst = err / bound
    print(f"{case} out: error {err:.3e} bound {bound:.3e}")
    assert err <= bound
    for call in (1, 2):   # the gradients are ADDED to what the buffers hold
        dev.bwd(full)
        worst = max(worst, check_grads(case, dev, call, g32, g64))

    if case.startswith("one_slab"):   # a workspace of one workgroup's states: one workgroup walks all four tiles through one slab
        one = Device(c)
        assert hip.instr_lstm_groups(one.desc, rows, one.slab) == 1 and tiles == 4 and gb == 4
        for call in (1, 2):
            one.bwd(one.slab)
            worst = max(worst, check_grads(case + " one slab", one, call, g32, g64))
    print(f"{case}: worst error / bound {worst:.3f}")


def test_refusals_write_nothing():
    """A workspace one byte short of one workgroup's states raises and writes nothing; ``rows = 0`` returns normally and writes
    nothing."""
    c, _, _ = reference("one_slab_h32")
    dev = Device(c)
    assert hip.instr_lstm_groups(dev.desc, dev.rows, dev.slab - 1) == 0 and hip.instr_lstm_groups(dev.desc, 0) == 0
    with pytest.raises(hip.HipError):
        dev.bwd(dev.slab - 1)
    assert all((t == 0.5).all() for t in dev.grads.values())
    assert (dev.fwd(rows=0) == 7.0).all()
    dev.bwd(dev.slab, rows=0)
    assert all((t == 0.5).all() for t in dev.grads.values())
