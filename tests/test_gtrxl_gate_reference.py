"""The formulas csrc/gtrxl_gate.hip computes -- the packing w_y = Wr | Wz | Wg, w_x = Ur | Uz | Ug, the sign of bg and the closed-form
backward of include/srl_hip.h, restated in tests/gtrxl_gate_ref.py -- against the real reference's GRUGatingUnit in float64
(tests/golden/gtrxl_gate.npz, written by tests/golden/gen_gtrxl_gate.py), and the sizes the library says it takes.  No device."""
import os

import numpy as np
import pytest
import torch

from gtrxl_gate_ref import gtrxl_gate
from srl_amd import hip

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gtrxl_gate.npz"))
REL = 1e-12


def test_restatement_matches_the_reference():
    t = lambda n: torch.from_numpy(GOLD[n])
    inp = dict(x=t("x"), y=t("y"), w_y=torch.cat([t("Wr"), t("Wz"), t("Wg")]), w_x=torch.cat([t("Ur"), t("Uz"), t("Ug")]), bg=t("bg"))
    got = gtrxl_gate(inp, t("dg"), torch.float64)
    want = dict(g=t("g"), dx=t("dx"), dy=t("dy"), d_bg=t("dbg"), dw_y=torch.cat([t("dWr"), t("dWz"), t("dWg")]),
                dw_x=torch.cat([t("dUr"), t("dUz"), t("dUg")]))
    assert float((t("bg") - 2).abs().max()) > 0.01
    for name, w in want.items():
        assert float((got[name] - w).abs().max()) <= REL * float(w.abs().max()), name


@pytest.mark.parametrize("D, ok", [(64, True), (128, True), (256, True), (32, False), (96, False), (512, False), (0, False)])
def test_supported_sizes(D, ok):
    assert hip.gtrxl_gate_supported(D) is ok
    assert (hip.gtrxl_gate_bwd_workspace(D, 5) > 0) is ok
    assert hip.gtrxl_gate_bwd_workspace(D, 0) == -1 and hip.gtrxl_gate_bwd_workspace(D, -3) == -1
