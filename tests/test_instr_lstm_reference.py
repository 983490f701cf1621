"""tests/instr_lstm_ref.py against the real reference's own modules (the golden blocks of tests/golden/instr_lstm_blocks.npz, float64
and float32 runs), and its deliberate faults against the float64 rule's bound at the shapes tests/test_gpu_instr_lstm.py runs.
CPU only."""
import functools

import numpy as np
import pytest
import torch

import instr_lstm_ref as ref
from dmlab_cases import BLOCKS, block_params, get64, unpack
from test_gpu_dmlab import bound64

# ten times the measured agreement or 1e-9, whichever is larger (measured: see the first test)
GOLDEN_TOL_OUT, GOLDEN_TOL_GRAD = 1e-9, 1.54e-9


def run_block(g, name, dtype):
    pre = f"blk_{name}_"
    return ref.encoder(block_params(g, name), g[pre + "tok"], g[pre + "cot"], dtype)


@pytest.mark.parametrize("name", BLOCKS + ("a0",))
def test_float64_statement_reproduces_the_golden_blocks(name, golden):
    """Output and every parameter gradient against the goldens' float64 values, relative to each tensor's largest element.
    Measured over the six blocks: at most 4.53e-11 for the output and 1.54e-10 for a gradient (block c, the table's: 5 rows of one
    step each), the resolution at which the goldens store their float64 values (an eleven-bit correction to the float32 run).
    So the output is held to 1e-9 and the gradients to ten times their measured worst, 1.54e-9."""
    g = golden("instr_lstm_blocks.npz")
    pre = f"blk_{name}_"
    out, grads = run_block(g, name, torch.float64)
    want = get64(g, pre + "out", pre + "out32")
    rel = np.abs(out - want).max() / np.abs(want).max()
    print(f"block {name} out: {rel:.2e} of the largest element")
    assert rel <= GOLDEN_TOL_OUT
    g64 = unpack(g, pre + "grad", f64=True)
    assert set(g64) == set(grads)
    for k, v in g64.items():
        err, top = np.abs(grads[k] - v).max(), np.abs(v).max()   # (rows of one step only: d W_hh is identically zero, in both)
        rel = err / top if top > 0 else (0.0 if err == 0 else np.inf)
        print(f"block {name} {k}: {rel:.2e} of the largest element")
        assert rel <= GOLDEN_TOL_GRAD, (k, rel)
    assert not grads[ref.EMB][0].any()   # row 0 of the table: read (case a0), never given gradient


@pytest.mark.parametrize("name", BLOCKS + ("a0",))
def test_float32_statement_lands_where_the_references_float32_run_does(name, golden):
    """The float32 run against the goldens' float32 output and gradients, within the float64 rule's bound."""
    g = golden("instr_lstm_blocks.npz")
    pre = f"blk_{name}_"
    out, grads = run_block(g, name, torch.float32)
    ref32, ref64 = g[pre + "out32"], get64(g, pre + "out", pre + "out32")
    err, bound = np.abs(out.astype(np.float64) - ref32).max(), bound64(ref32, ref64)
    print(f"block {name} out: difference {err:.3e} bound {bound:.3e}")
    assert err <= bound
    g32, g64 = unpack(g, pre + "grad"), unpack(g, pre + "grad", f64=True)
    for k, v in g32.items():
        err, bound = np.abs(grads[k].astype(np.float64) - v).max(), bound64(v, g64[k])
        print(f"block {name} {k}: difference {err:.3e} bound {bound:.3e}")
        assert err <= bound, (k, err, bound)


def test_tokens_are_read_as_the_kernel_reads_them():
    tok = np.array([[30, 3, -2, 1e9, 0, 0], [4, 37, 6, 0, 0, 0], [0.5, np.nan, 3.9, 0, 0, 29.99]], np.float32)
    want = [[0, 3, 0, 0, 0, 0], [4, 0, 6, 0, 0, 0], [0, 0, 3, 0, 0, 29]]
    assert ref.read_tokens(tok, 30).tolist() == want
    assert ref.read_tokens(np.array([[30, 3, -2, 29]], np.int32), 30).tolist() == [[0, 3, 0, 29]]


def test_library_reports_the_grid_a_workspace_leaves():
    """``hip.instr_lstm_groups`` needs the library, not a device: 101 rows are four tiles; a workspace of one workgroup's states
    leaves one workgroup, a byte less none (the backward refuses it)."""
    from srl_amd import hip
    for V, Ed, H, L in ref.CASES.values():
        d = hip.instr_lstm_desc(V, Ed, H, L)
        slab = 2 * L * H * 32 * 4
        assert hip.instr_lstm_bwd_workspace(d, 101) == 4 * slab
        assert hip.instr_lstm_groups(d, 101) == hip.instr_lstm_groups(d, 101, 4 * slab) == hip.instr_lstm_groups(d, 101, 9 * slab) == 4
        assert hip.instr_lstm_groups(d, 101, 3 * slab - 1) == 2 and hip.instr_lstm_groups(d, 101, slab) == 1
        assert hip.instr_lstm_groups(d, 101, slab - 1) == 0 and hip.instr_lstm_groups(d, 0) == 0
    assert hip.instr_lstm_groups(hip.instr_lstm_desc(1000, 20, 48, 12), 101) == 0   # an unsupported shape


ROWS, FAULT_ROW = 200, 128   # the GPU cases' row counts cut to a few hundred; the "second round" starts at row 128


@functools.lru_cache(maxsize=None)
def honest(case):
    c = ref.draw_case(case, ROWS, seed=7)
    return c, ref.encoder(c["params"], c["tok"], c["cot"], torch.float32), ref.encoder(c["params"], c["tok"], c["cot"], torch.float64)


@pytest.mark.parametrize("fault", ref.FAULTS)
@pytest.mark.parametrize("case", ref.CASES)
def test_every_fault_breaks_the_bound(case, fault):
    """The faulty float64 result violates ``bound64`` of the honest float32 and float64 runs in some tensor, at every GPU case's
    shape (fewer rows)."""
    c, (out32, g32), (out64, g64) = honest(case)
    out, grads = ref.encoder(c["params"], c["tok"], c["cot"], torch.float64, fault=fault, fault_row=FAULT_ROW)
    rows = [("out", np.abs(out - out64).max(), bound64(out32, out64))]
    rows += [(k, np.abs(grads[k] - g64[k]).max(), bound64(g32[k], g64[k])) for k in g64]
    broken = [r for r in rows if not r[1] <= r[2]]
    print(f"{case} {fault}: over the bound (tensor, error, bound): {broken[:3]}")
    assert broken, (case, fault, max(rows, key=lambda r: r[1] / r[2]))


def test_drawn_cases_hold_rows_of_every_kind():
    for case in ref.CASES:
        c, (out32, _), (out64, g64) = honest(case)
        V, L, tok = c["V"], c["L"], c["tok"]
        read = ref.read_tokens(tok, V)
        cnt = (read != 0).sum(1)
        assert (cnt == 0).any() and (cnt == L).any() and cnt[ROWS - 1] == L
        assert any(n >= 2 and (read[i, :n] == 0).any() for i, n in enumerate(cnt))                  # a zero inside a prefix
        assert any(n < L and (read[i, n:] != 0).any() for i, n in enumerate(cnt))                    # a token behind a gap
        bad = ~((tok >= 0) & (tok < V))
        assert bad.any() and not c["cot"][bad.any(1)].any()                                          # out-of-range: no gradient
        assert not g64[ref.EMB][0].any() and c["params"][ref.EMB][0].any()
        print(f"{case}: float32 output error {np.abs(out32 - out64).max() / np.abs(out64).max():.2e} of the largest element")
