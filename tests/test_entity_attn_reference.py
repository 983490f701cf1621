"""tests/entity_attn_ref.py against the real reference's own modules (the golden blocks of tests/golden/steps_smac_attn.npz, float64
and float32 runs), and its deliberate faults against the float64 rule's bound at the shapes tests/test_gpu_entity_attn.py runs.
CPU only."""
import functools

import numpy as np
import pytest
import torch

import entity_attn_ref as ref
from smac_attn_cases import BLOCKS, get64, unpack
from test_gpu_smac_attn import bound64

KBIAS, QBIAS = "encoder.attn.k_linear.bias", "encoder.attn.q_linear.bias"


def run_block(g, name, dtype):
    pre = f"blk_{name}_"
    keys = [str(k) for k in g[pre + "keys"]]
    return ref.encoder(unpack(g, pre + "param"), g[pre + "x.obs_self"], [g[pre + "x." + k] for k in keys], g[pre + "mask"], g[pre + "cot"],
                       keys, dtype)[:2]


@pytest.mark.parametrize("name", BLOCKS)
def test_float64_statement_reproduces_the_golden_blocks(name, golden):
    """Output and every parameter gradient within 1e-9 of each tensor's largest element (measured: 5.0e-11 and 1.6e-10, the
    resolution at which the goldens store their float64 values); ``k_linear.bias``, whose true gradient is zero, takes its scale
    from ``q_linear.bias``."""
    g = golden("steps_smac_attn.npz")
    pre = f"blk_{name}_"
    out, grads = run_block(g, name, torch.float64)
    want = get64(g, pre + "out", pre + "out32")
    rel = np.abs(out - want).max() / np.abs(want).max()
    print(f"block {name} out: {rel:.2e} of the largest element")
    assert rel <= 1e-9
    g64 = unpack(g, pre + "grad", f64=True)
    assert set(g64) == set(grads)
    for k, v in g64.items():
        rel = np.abs(grads[k] - v).max() / np.abs(g64[QBIAS] if k == KBIAS else v).max()
        print(f"block {name} {k}: {rel:.2e} of the largest element")
        assert rel <= 1e-9, (k, rel)


@pytest.mark.parametrize("name", BLOCKS)
def test_float32_statement_lands_where_the_references_float32_run_does(name, golden):
    """The float32 run against the goldens' float32 output and gradients, within the float64 rule's bound."""
    g = golden("steps_smac_attn.npz")
    pre = f"blk_{name}_"
    out, grads = run_block(g, name, torch.float32)
    ref32, ref64 = g[pre + "out32"], get64(g, pre + "out", pre + "out32")
    err, bound = np.abs(out.astype(np.float64) - ref32).max(), bound64(ref32, ref64)
    print(f"block {name} out: difference {err:.3e} bound {bound:.3e}")
    assert err <= bound
    g32, g64 = unpack(g, pre + "grad"), unpack(g, pre + "grad", f64=True)
    for k, v in g32.items():
        err, bound = np.abs(grads[k].astype(np.float64) - v).max(), bound64(v, g64[k], g64[QBIAS] if k == KBIAS else None)
        print(f"block {name} {k}: difference {err:.3e} bound {bound:.3e}")
        assert err <= bound, (k, err, bound)


@pytest.mark.parametrize("case", ref.CASES)
def test_library_plans_the_staging_each_case_stands_for(case):
    """``hip.entity_attn_plan`` needs the library, not a device: the backward plan of every GPU case stages what the case is there
    to reach (rows per tile and staging do not depend on the device; the grid does, and is left to the GPU test)."""
    from srl_amd import hip
    D, S, shapes, staging = ref.CASES[case]
    fwd, bwd = (hip.entity_attn_plan(D, S, shapes, b, 1000) for b in (0, 1))
    print(f"{case}: forward {fwd} backward {bwd}")
    assert (bwd["stage_p"], bwd["stage_g"]) == staging and (fwd["stage_p"], fwd["stage_g"]) == (staging[0], 0)
    for p in (fwd, bwd):
        assert 1 <= p["R"] <= 16 and p["lds"] <= 160 * 1024 and p["tiles"] == -(-1000 // p["R"]) and 1 <= p["groups"] <= p["tiles"]
    assert hip.entity_attn_plan(D, S, shapes, 1, 0)["groups"] == 0
    with pytest.raises(hip.HipError):   # what the launch refuses, the query refuses
        hip.entity_attn_plan(D + 1, S, shapes, 0, 10)
    with pytest.raises(hip.HipError):
        hip.entity_attn_plan(D, S, shapes, 1, -1)


ROWS, FAULT_ROW = 200, 120  # the GPU cases' row counts cut to a few hundred; the "second round" starts at row 120
# A fault that IS the honest computation at a shape leaves the bound nothing to catch.  With one entity the only query is its own
# only key: a masked query's attention output is already 0 (p * mask_key), so pooling it in or not is the same arithmetic.
IDENTITIES = {("smallest", "masked_query_pooled")}


@functools.lru_cache(maxsize=None)
def honest(case):
    c = ref.draw_case(case, ROWS, seed=7, forced=(FAULT_ROW,))
    args = (c["params"], c["x_self"], c["x_keys"], c["mask"], c["cot"], c["keys"])
    return c, args, ref.encoder(*args, torch.float32)[:2], ref.encoder(*args, torch.float64)[:2]


@pytest.mark.parametrize("fault", ref.FAULTS)
@pytest.mark.parametrize("case", ref.CASES)
def test_every_fault_breaks_the_bound(case, fault):
    """The faulty float64 result violates ``bound64`` of the honest float32 and float64 runs in some tensor, at every GPU case's
    shape (fewer rows)."""
    c, args, (out32, g32), (out64, g64) = honest(case)
    out, grads = ref.encoder(*args, torch.float64, fault=fault, fault_row=FAULT_ROW)[:2]
    if all(np.array_equal(grads[k], g64[k]) for k in g64) and np.array_equal(out, out64):
        assert (case, fault) in IDENTITIES, "the fault changes nothing here"
        return
    assert (case, fault) not in IDENTITIES
    floors = ref.zero_gradient_floors(c["S"], c["shapes"])
    rows = [("out", np.abs(out - out64).max(), bound64(out32, out64))]
    rows += [(k, np.abs(grads[k] - g64[k]).max(), bound64(g32[k], g64[k], g64[floors[k]] if k in floors else None)) for k in g64]
    broken = [r for r in rows if not r[1] <= r[2]]
    print(f"{case} {fault}: over the bound (tensor, error, bound): {broken[:3]}")
    assert broken, (case, fault, max(rows, key=lambda r: r[1] / r[2]))


def test_honest_runs_hold_their_own_bound_and_the_gate_filter_drops_little():
    """The float32 statement is inside the bound it sets (so a violation above is the fault's), and ``draw_case`` asserts that at
    most 20 % of the drawn rows fall to the gate filter; all-masked rows pool to exactly 0."""
    for case in ref.CASES:
        c, _, (out32, _), (out64, _) = honest(case)
        D = c["D"]
        print(f"{case}: gate filter dropped {100 * c['dropped']:.1f} % of the drawn rows; float32 output error "
              f"{np.abs(out32 - out64).max() / np.abs(out64).max():.2e} of the largest element")
        empty = c["mask"].sum(1) == 0
        assert empty[[0, FAULT_ROW, ROWS - 1]].all() and c["mask"][1].sum() == 1
        assert (out64[empty, D:] == 0).all() and (out32[empty, D:] == 0).all()
