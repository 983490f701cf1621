"""tests/gae_ref.py and tests/gae_cases.py without a GPU (the library is loaded for `srl_gae_scan_plan`, no device is touched):

* `gae_ref.gae`, rounded once, is the oracle (oracle/gae.py) and the real reference's recorded outputs (tests/golden/gae*.npz) bit
  for bit;
* the kernels' evaluation order (`gae_ref.scan_in_tiles` at the plan of every GPU case) stays inside the float64 term of the bound
  -- re-association alone cannot break it.  Worst |scan - g| / (4 T 2^-53 A) over all cases: 0.24 (reg64_L1_B98304_T4: the term
  grows with T, so the shortest scans over the most columns come closest); T = 5 on 786 432 columns 0.22; every case with
  T >= 128 sits below 0.01;
* every deliberate fault of `gae_ref.FAULTS` breaks the bound on every GPU case it applies to (`applies` states the rule), and each
  is shown by at least one case of every kernel it concerns;
* the case list reaches every branch of the launch choice, by the plan."""
import numpy as np
import pytest

import gae_cases as gc
import gae_ref
from gae_cases import LDS, REG
from oracle import gae as ogae
from srl_amd import hip

CONCERNS = {f: (REG, LDS) for f in gae_ref.FAULTS}
CONCERNS.update(done_rotated_in_quad=(REG,), tensors_from_tile_row0=(LDS,), flag_col_not_divided=(LDS,))


def applies(fault, case, plan) -> bool:
    """Whether `case` can show `fault` at all."""
    first_tile = case.T - gc.tile_starts(case.T, plan)[0]
    return {
        "no_done_mask": True,
        "done_rotated_in_quad": plan["kernel"] == REG,                 # the byte picks exist in the register kernel only
        "truncated_ignored": case.T >= 2,                              # m[t] multiplies adv[t + 1], and adv[T] = 0
        "on_reset_same_row": True,
        "rho_c_swapped": case.vtrace,
        "tensors_from_tile_row0": case.tensors and plan["tiles"] > 1,  # t0 = 0 in the only tile of a one-tile case
        "flag_col_not_divided": case.Nc > 1,
        "carry_zeroed_at_tile_seam": plan["tiles"] > 1,
        "carry_from_wrong_chunk": first_tile > gc.chunk_rows(case.T, plan),   # two chunks with rows in one tile
    }[fault]


def scan_of(r, plan, fault=None):
    if plan["kernel"] == REG:
        return gae_ref.scan_in_tiles(r["delta"], r["m"], gc.seg_of(plan), plan["L"], fault=fault)
    return gae_ref.scan_in_tiles(r["delta"], r["m"], gc.seg_of(plan), None, TT=plan["TT"], log_step=False, fault=fault)


# ------------------------------------------------------------------------------------------------ the reference itself
def _golden_blocks(golden):
    g = golden("gae.npz")
    for name in g["cases"]:
        arr = [g[f"{name}_{k}"] for k in ("reward", "value", "done", "truncated", "on_reset")]
        for tag, gam, lam in (("a", 0.99, 0.97), ("b", 0.9, 0.5)):
            yield f"{name}_{tag}", arr, gam, lam, None, g[f"{name}_{tag}_adv"], g[f"{name}_{tag}_ret"]
        yield f"{name}_vtrace", arr, 0.99, 0.97, g[f"{name}_ratio"], g[f"{name}_vtrace_adv"], None
    g = golden("gae_tensor.npz")
    for name in g["cases"]:
        arr = [g[f"{name}_{k}"] for k in ("reward", "value", "done", "truncated", "on_reset")]
        gam, lam = g[f"{name}_gamma"], g[f"{name}_lambda"]
        for tag, gg, ll in (("gl", gam, lam), ("g", gam, 0.95), ("l", 0.99, lam)):
            yield f"{name}_{tag}", arr, gg, ll, None, g[f"{name}_{tag}_adv"], None
        yield f"{name}_vtrace", arr, gam, lam, g[f"{name}_ratio"], g[f"{name}_vtrace_adv"], None


def test_reference_reproduces_the_golden_blocks(golden):
    n = 0
    for tag, arr, gam, lam, ratio, adv, ret in _golden_blocks(golden):
        r = gae_ref.gae(*arr, gam, lam, ratio=ratio)
        a32 = r["g"].astype(np.float32)
        assert np.array_equal(a32, adv), tag
        if ret is not None:
            assert np.array_equal(a32 + r["v"][:-1], ret), tag
        assert (r["A"] >= np.abs(r["g"])).all()
        n += 1
    assert n == 4 * 3 + 3 * 4
    # the hand-computed vector of the reference's own test (legacy/tests/modules_test.py:119-138): its value is 0 on its done row
    g = golden("gae.npz")
    shp = lambda k, dt: g[f"hand_{k}"].reshape(-1, 1, 1).astype(dt)
    r = gae_ref.gae(shp("reward", np.float32), shp("value", np.float32), shp("done", np.uint8), shp("truncated", np.uint8),
                    shp("on_reset", np.uint8), 0.1, 0.1)
    assert np.array_equal(r["g"].astype(np.float32)[:, 0, 0], g["hand_adv"])
    keep = 1 - g["hand_on_reset"][1:]
    np.testing.assert_array_almost_equal(r["g"][:, 0, 0] * keep, np.array([2.1 * 0.01 - 1, 2.1, 0, -0.8 + 0.01, 1, 0, 0.111, 1.1]) * keep)


def test_stats_counts_the_mask_once_per_step_and_env():
    rng = np.random.default_rng(0)
    adv = rng.standard_normal((5, 3, 2)).astype(np.float32)
    on_reset = (rng.random((6, 3, 1)) < 0.4).astype(np.uint8)
    s = gae_ref.stats(adv, on_reset)
    mask = 1.0 - on_reset[1:, :, 0]
    x = adv.astype(np.float64) * mask[..., None]
    assert s["n"] == mask.sum() and s["s"] == pytest.approx(x.sum(), rel=1e-15) and s["q"] == pytest.approx((x ** 2).sum(), rel=1e-15)
    assert s["sabs"] == pytest.approx(np.abs(x).sum(), rel=1e-15)


def test_scan_in_tiles_is_the_recurrence_for_every_tiling():
    """Exact data (small integers, m in {0, 1/2, 1}): every association order gives the same float64, so any tiling must be bit-equal
    to the sequential recurrence -- and every scan fault must not be."""
    rng = np.random.default_rng(1)
    delta = rng.integers(-4, 5, size=(45, 6)).astype(np.float64)
    m = rng.choice([0.0, 0.5, 1.0], p=[0.1, 0.6, 0.3], size=(45, 6))
    g = np.zeros_like(delta)
    run = np.zeros(6)
    for t in range(44, -1, -1):
        run = delta[t] + m[t] * run
        g[t] = run
    for SEG in (1, 2, 4, 8, 64):
        for L in (1, 2, 4):
            assert np.array_equal(gae_ref.scan_in_tiles(delta, m, SEG, L), g), (SEG, L)
            assert not np.array_equal(gae_ref.scan_in_tiles(delta, m, 4, L, fault="carry_zeroed_at_tile_seam"), g)
            assert not np.array_equal(gae_ref.scan_in_tiles(delta, m, 4, L, fault="carry_from_wrong_chunk"), g)
        for TT in (45, 23, 8):
            assert np.array_equal(gae_ref.scan_in_tiles(delta, m, SEG, None, TT=TT, log_step=False), g), (SEG, TT)
    assert not np.array_equal(gae_ref.scan_in_tiles(delta, m, 4, None, TT=23, log_step=False, fault="carry_zeroed_at_tile_seam"), g)
    assert not np.array_equal(gae_ref.scan_in_tiles(delta, m, 4, None, TT=23, log_step=False, fault="carry_from_wrong_chunk"), g)


# ------------------------------------------------------------------------------------------------ the cases
def test_plan_entry_point():
    p = hip.gae_scan_plan(128, 4096)
    assert p == dict(kernel=0, width=8, L=4, TT=128, tiles=1, grid=128, workspace=1)
    assert hip.gae_scan_plan(128, 4096, aligned=False)["kernel"] == 1 and hip.gae_scan_plan(128, 4096, tensors=True)["kernel"] == 1
    assert hip.gae_scan_plan(128, 4096, Nc=2)["kernel"] == 1 and hip.gae_scan_plan(128, 4095)["kernel"] == 1
    assert hip.gae_scan_plan(0, 64)["grid"] == 0 and hip.gae_scan_plan(64, 0)["grid"] == 0
    with pytest.raises(hip.HipError):
        hip.gae_scan_plan(-1, 4)
    with pytest.raises(hip.HipError):
        hip.gae_scan_plan(4, 4, Nc=0)


def test_case_list_covers_every_branch():
    plans = {c.name: gc.plan_of(c) for c in gc.CASES}
    for c in gc.CASES:
        gc.assert_on_branch(c, plans[c.name])
    reg = [(c, plans[c.name]) for c in gc.CASES if plans[c.name]["kernel"] == REG]
    lds = [(c, plans[c.name]) for c in gc.CASES if plans[c.name]["kernel"] == LDS]
    # every register width x every L it can take, single-tile; one multi-tile case per width, with and without V-trace
    assert {(p["width"], p["L"]) for c, p in reg if p["tiles"] == 1} >= {(w, L) for w, Ls in gc.REG_WIDTHS.items() for L in Ls}
    for vt in (False, True):
        assert {p["width"] for c, p in reg if p["tiles"] > 1 and c.T % p["TT"] and c.vtrace == vt} == set(gc.REG_WIDTHS)
    # part-filled last workgroup, one quad
    assert any(c.B % (4 * p["width"]) for c, p in reg if p["grid"] > 1) and any(c.B == 4 for c, p in reg)
    # both LDS widths single- and multi-tile; the four feature combinations multi-tile; channels; a quad layout with a tensor
    assert {(p["width"], p["tiles"] > 1) for c, p in lds} == {(w, m) for w in gc.LDS_WIDTHS for m in (False, True)}
    assert {(c.vtrace, c.tensors) for c, p in lds if p["tiles"] > 1} == {(v, t) for v in (False, True) for t in (False, True)}
    assert {(c.gamma_t, c.lambda_t) for c, p in lds if p["tiles"] > 1} >= {(True, False), (False, True), (True, True)}
    assert {c.Nc for c, p in lds} >= {1, 2, 3}
    assert any(c.B % 4 == 0 and c.Nc == 1 and c.tensors and not c.misalign for c, p in lds)
    assert {(c.misalign, hip.gae_scan_plan(c.T, c.B)["width"]) for c, p in lds if c.misalign} == {(m, w) for m in ("value", "done") for w in (4, 32)}
    # T = 1 and a free-flags case on both kernels; the second (gamma, lambda) pair on both
    for group in (reg, lds):
        assert any(c.T == 1 for c, p in group) and any(c.free_flags for c, p in group) and any(c.gl == (0.9, 0.5) for c, p in group)
    # every fault has a case of every kernel it concerns
    for fault, kernels in CONCERNS.items():
        for k in kernels:
            assert any(applies(fault, c, p) for c, p in (reg if k == REG else lds)), (fault, k)


@pytest.mark.parametrize("name", [c.name for c in gc.CASES])
def test_case_reference_scan_order_and_faults(name):
    case = gc.BY_NAME[name]
    plan = gc.plan_of(case)
    a = gc.build(case, plan)
    gc.check_inputs(case, a)
    T = case.T
    r = gc.reference(a)
    g, A = r["g"], r["A"]
    # one rounding of the reference is the oracle, bit for bit
    kw = dict(vtrace=True, imp_ratio=a["ratio"], rho=a["rho"], c=a["c"]) if case.vtrace else {}
    o_adv, o_ret = ogae.adv_and_value_target(a["reward"], a["value"], a["truncated"], a["done"], a["on_reset"], a["gamma"], a["lmbda"], **kw)
    assert np.array_equal(g.astype(np.float32), o_adv) and np.array_equal(g.astype(np.float32) + r["v"][:-1], o_ret)
    assert (A >= np.abs(g)).all()
    # the kernel's order stays inside the float64 term
    err = np.abs(scan_of(r, plan) - g)
    term = gae_ref.f64_term(A, T)
    assert (err <= term).all()
    worst = float((err[term > 0] / term[term > 0]).max())
    print(f"{name}: scan_in_tiles worst |scan - g| / float64 term = {worst:.4f}")
    # every fault that applies breaks the bound
    bnd = gae_ref.bound(g, A, T)
    for fault in gae_ref.FAULTS:
        if not applies(fault, case, plan):
            continue
        if fault in gae_ref.SCAN_FAULTS:
            bad = scan_of(r, plan, fault=fault)
        else:
            bad = scan_of(gc.reference(a, fault=fault, TT=plan["TT"]), plan)
        bad = bad.astype(np.float32).astype(np.float64)
        assert (np.abs(bad - g) > bnd).any(), (name, fault)
