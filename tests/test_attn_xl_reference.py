"""The formula csrc/attn_xl.hip computes -- the closed-form relative shift r[j + C - 1 - i] and the causal-with-memory mask of
include/srl_hip.h, restated in tests/attn_xl_ref.py -- against the real reference's AttentionXL in float64
(tests/golden/attn_xl.npz, written by tests/golden/gen_attn_xl.py), and the sizes the library says it takes.  No device."""
import os

import numpy as np
import pytest
import torch

from attn_xl_ref import NAMES, attn_xl_grads
from srl_amd import hip

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_xl.npz"))
REL = 1e-12


@pytest.mark.parametrize("ci", range(len(GOLD["cases"])), ids=lambda ci: "-".join(map(str, GOLD["cases"][ci])))
def test_restatement_matches_the_reference(ci):
    t = lambda n: torch.from_numpy(GOLD[f"c{ci}_{n}"])
    got = attn_xl_grads({n: t(n) for n in NAMES}, t("g"), torch.float64)
    got["y"] = got.pop("out") @ t("project_w").T + t("project_b")   # the module's output: the attention vector through `project`
    assert float(t("u").abs().min()) > 0 and float(t("v").abs().min()) > 0
    for name, x in got.items():
        want = t(name)
        assert float((x - want).abs().max()) <= REL * float(want.abs().max()), name


@pytest.mark.parametrize("shape, ok", [((4, 8, 4, 4), False), ((4, 16, 1, 192), False), ((4, 16, 64, 128), True), ((1, 16, 1, 0), True),
                                       ((8, 64, 64, 0), True), ((9, 16, 4, 4), False), ((4, 32, 65, 0), False), ((4, 32, 4, -1), False)],
                         ids=str)
def test_supported_sizes(shape, ok):
    """(nh, dh, C, M): dh = 8 no, F = 193 no, F = 192 yes, C = 1 with M = 0 yes; the workspace answers -1 where it is no."""
    assert hip.attn_xl_supported(*shape) is ok
    assert (hip.attn_xl_bwd_workspace(*shape, 5) > 0) is ok
