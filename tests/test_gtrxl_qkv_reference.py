"""The formulas csrc/gtrxl_qkv.hip computes -- keep o memory || inputs, LayerNorm over ALL rows, key | value from the normalised rows,
q from the raw inputs, and the closed-form backward of include/srl_hip.h with dgamma / dbeta through the memory rows, restated in
tests/gtrxl_qkv_ref.py -- against the real reference's layernorm1 / attention_kv / attention_q in float64
(tests/golden/gtrxl_qkv.npz, written by tests/golden/gen_gtrxl_qkv.py), and the sizes the library says it takes.  No device."""
import os

import numpy as np
import pytest
import torch

from gtrxl_qkv_ref import NAMES, gtrxl_qkv
from srl_amd import hip

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gtrxl_qkv.npz"))
REL = 1e-12


def test_restatement_matches_the_reference():
    t = lambda n: torch.from_numpy(GOLD[n])
    assert sorted(t("keep").tolist()) == [0, 1, 1, 1, 1] and float((t("gamma") - 1).abs().max()) > 0.1
    got = gtrxl_qkv({n: t(n) for n in NAMES + ("keep",)}, t("dkv"), t("dq"), torch.float64)
    for name in ("kv", "q", "x1", "dx", "dgamma", "dbeta", "db_kv", "db_q", "dw_kv", "dw_q"):
        w = t(name)
        assert float((got[name] - w).abs().max()) <= REL * float(w.abs().max()), name


@pytest.mark.parametrize("D, ok", [(64, True), (128, True), (256, True), (32, False), (96, False), (512, False), (0, False)])
def test_supported_sizes(D, ok):
    assert hip.gtrxl_qkv_supported(D) is ok
    assert (hip.gtrxl_qkv_bwd_workspace(D, 5) == 5 * D * 4) is ok and (hip.gtrxl_qkv_bwd_workspace(D, 1 << 30) == 256 * 5 * D * 4) is ok
    assert hip.gtrxl_qkv_bwd_workspace(D, 0) == -1 and hip.gtrxl_qkv_bwd_workspace(D, -3) == -1
