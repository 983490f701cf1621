"""The fused attention encoder (csrc/entity_attn.hip) beyond a workgroup's first tile: seeded cases on every staging outcome of the
backward plan, each with enough rows that every workgroup of the persistent grid takes a second tile, one a third, and the last
tile is ragged -- against the float64 restatement (tests/entity_attn_ref.py), every element, by the project's rule: an error of at
most 3 x the float32 statement's own error plus 2e-6 of the tensor's largest float64 element, per tensor, on the same rows.

Every case is a mutation test in all but name: leaves, ``d_out`` and ``out`` have padded pitches and 8 guard rows behind the rows the
kernel is told about (NaN where it must not read, 7.0 where it must not write), the gradient buffers start at 0.5 and take two
backward calls, and rows 0, the last one and the first one of the grid's second round are all-masked."""
import functools

import numpy as np
import pytest
import torch

import entity_attn_ref as ref
import srl_amd
from srl_amd import hip
from test_gpu_smac_attn import SLOTS, bound64

srl_amd.register_all()
pytestmark = pytest.mark.gpu

PAD, GUARD = 3, 8


def plan_rows(D, S, shapes):
    """(rows, forward plan, backward plan): two full rounds of the larger grid, one more tile and a ragged rest, from the
    library's own plan (never hard-coded)."""
    full = [hip.entity_attn_plan(D, S, shapes, bwd, 1 << 24) for bwd in (0, 1)]   # (so many rows that the grid is at its cap)
    big = max(full, key=lambda p: p["R"] * p["groups"])
    rows = 2 * big["R"] * big["groups"] + big["R"] + (min(5, big["R"] - 1) if big["R"] > 1 else 2)
    return rows, hip.entity_attn_plan(D, S, shapes, 0, rows), hip.entity_attn_plan(D, S, shapes, 1, rows)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's data and the float32 / float64 statements of it, computed once."""
    D, S, shapes, _ = ref.CASES[case]
    rows, pf, pb = plan_rows(D, S, shapes)
    c = ref.draw_case(case, rows, seed=20 + list(ref.CASES).index(case), forced=(pf["R"] * pf["groups"], pb["R"] * pb["groups"]))
    args = (c["params"], c["x_self"], c["x_keys"], c["mask"], c["cot"], c["keys"])
    return c, rows, pf, pb, ref.encoder(*args, torch.float32)[:2], ref.encoder(*args, torch.float64)[:2]


def padded(a, fill, dtype=torch.float32):
    """[n, w] -> device [n + GUARD, w + PAD] holding ``fill`` around the array."""
    n, w = a.shape
    t = torch.full((n + GUARD, w + PAD), fill, dtype=dtype)
    t[:n, :w] = torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda()


@pytest.mark.parametrize("case", ref.CASES)
def test_case_vs_float64(case):
    c, rows, pf, pb, (out32, g32), (out64, g64) = reference(case)
    D, S, shapes, keys, E = c["D"], c["S"], c["shapes"], c["keys"], c["mask"].shape[1]
    print(f"\n{case}: rows {rows}, gate filter dropped {100 * c['dropped']:.1f} %, forward plan {pf}, backward plan {pb}")
    assert hip.entity_attn_supported(D, S, shapes)
    assert (pb["stage_p"], pb["stage_g"]) == ref.CASES[case][3] and pf["stage_p"] == pb["stage_p"] and pf["stage_g"] == 0
    for p in (pf, pb):   # every workgroup takes a second tile, one takes a third, and the last tile is ragged
        assert p["tiles"] >= 2 * p["groups"] + 1 and (p["R"] == 1 or rows % p["R"] != 0), p
    empty = c["mask"].sum(1) == 0
    assert empty[[0, rows - 1, pf["R"] * pf["groups"], pb["R"] * pb["groups"]]].all() and c["mask"][1].sum() == 1

    params = {k: torch.from_numpy(v).cuda() for k, v in c["params"].items()}
    grads = {k: torch.full_like(v, 0.5) for k, v in params.items()}
    slots = dict(SLOTS)
    for i, k in enumerate(keys):
        slots[f"{k}_norm"] = (hip.EATTN_LN_KEY_W + i, hip.EATTN_LN_KEY_B + i)
        slots[f"encoder.embedding.{k}_fc.0"] = (hip.EATTN_KEY_W + i, hip.EATTN_KEY_B + i)
    p, gr = {}, {}
    for prefix, (sw, sb) in slots.items():
        for slot, what in ((sw, "weight"), (sb, "bias")):
            p[slot], gr[slot] = params[f"{prefix}.{what}"].data_ptr(), grads[f"{prefix}.{what}"].data_ptr()
    assert len(p) == len(params)
    desc = hip.entity_attn_desc(D, S, shapes, p, gr)
    x_self = padded(c["x_self"], np.nan)
    x_keys = [padded(x.reshape(rows, -1), np.nan) for x in c["x_keys"]]
    mask = padded(c["mask"], 1, torch.uint8)
    cot = padded(c["cot"], np.nan)
    leaves = ((x_self.data_ptr(), S + PAD), [(x.data_ptr(), x.shape[1]) for x in x_keys], (mask.data_ptr(), E + PAD))
    ldo = 2 * D + PAD
    out = torch.full((rows + GUARD, ldo), 7.0, dtype=torch.float32, device="cuda")

    hip.entity_attn_fwd(desc, *leaves, 0, out.data_ptr(), ldo)   # rows = 0: returns normally and writes nothing
    hip.entity_attn_bwd(desc, *leaves, 0, cot.data_ptr(), ldo)
    assert (out == 7.0).all() and all((t == 0.5).all() for t in grads.values())

    hip.entity_attn_fwd(desc, *leaves, rows, out.data_ptr(), ldo)
    got = out.cpu().numpy()
    assert (got[:rows, 2 * D:] == 7.0).all() and (got[rows:] == 7.0).all()   # pad columns and guard rows stay
    got = got[:rows, :2 * D]
    err, bound = np.abs(got - out64).max(), bound64(out32, out64)
    worst = err / bound
    print(f"{case} out: error {err:.3e} bound {bound:.3e}")
    assert err <= bound
    assert (got[empty, D:] == 0.0).all() and (out64[empty, D:] == 0.0).all()   # a row without entities pools to exactly 0

    floors = ref.zero_gradient_floors(S, shapes)
    for call in (1, 2):   # the gradients are ADDED to what the buffers hold
        hip.entity_attn_bwd(desc, *leaves, rows, cot.data_ptr(), ldo)
        for k, t in grads.items():
            floor = g64[floors[k]] if k in floors else None
            err, bound = np.abs(t.cpu().numpy().astype(np.float64) - 0.5 - call * g64[k]).max(), call * bound64(g32[k], g64[k], floor)
            worst = max(worst, err / bound)
            print(f"{case} call {call} {k}: error {err:.3e} bound {bound:.3e}")
            assert err <= bound, (k, call, err, bound)
    assert (out.cpu().numpy()[:rows, :2 * D] == got).all()   # the backward writes no output
    print(f"{case}: worst error / bound {worst:.3f}")

