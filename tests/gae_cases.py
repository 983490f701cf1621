"""The cases `srl_gae_scan` is held to float64 on (tests/test_gpu_gae.py), and their inputs.  Host-only: the tiling of a case is
asked of the library (`hip.gae_scan_plan`, the function the launch uses), never assumed from the thresholds; the GPU test asserts
that each case ran the branch it names, tests/test_gae_reference.py that the list covers every branch and that every deliberate
fault of tests/gae_ref.py breaks the bound on these very inputs.

Inputs.  `value` is drawn independently of `done` (the kernel's own `value * (1 - done)` has something to mask); rewards are drawn
and masked like `synthetic.make_sample_arrays`; V-trace cases use rho = 1.5, c = 1.2 with ratios in [0.3, 1.8), so both clamps bite
and differ; per-step tensors are float32 in [0.9, 1).  Flags are `synthetic.make_flags` plus a deterministic overlay computed from
the plan (`seam_rows`): each of done / truncated / on_reset lands on both sides of every time-tile seam, on both sides of one chunk
seam, on row 0, row T - 1 and the bootstrap row T, in three adjacent columns of one quad, so that the quad carries four different
flag patterns on that row.  The invariants of `oracle.gae.check_invariants` hold.  The two *free-flags* cases draw the three flags
independently (p = 0.1 each, truncated and on_reset allowed together): no invariant holds, the formulas of srl_hip.h alone define
the result."""
import zlib
from typing import NamedTuple, Optional

import numpy as np

import gae_ref
from srl_amd import hip
from srl_amd.runtime import synthetic

REG, LDS = 0, 1
REG_WIDTHS = {4: (1, 2, 4), 8: (1, 2, 4), 32: (1, 2, 4), 64: (1, 2, 4), 128: (1, 2), 256: (1, 2)}   # CQ -> the L it can take
LDS_WIDTHS = (16, 64)
RHO, C = 1.5, 1.2


class Case(NamedTuple):
    name: str
    kernel: int            # the branch the case is for: REG / LDS,
    width: int             # CQ / COLS,
    L: int                 # rows per lane (0: LDS),
    multi: bool            # more than one time tile (register kernel: the tile holding row 0 is then partial)
    T: int
    B: int
    Nc: int = 1
    vtrace: bool = False
    gamma_t: bool = False
    lambda_t: bool = False
    gl: tuple = (0.99, 0.97)
    misalign: Optional[str] = None   # "value": the leaf starts 4 bytes off a 16-byte boundary; "done": 1 byte off a 4-byte one
    free_flags: bool = False

    @property
    def tensors(self):
        return self.gamma_t or self.lambda_t


def _reg(width, B, Ts, **kw):
    """L = 1 / 2 / 4 single-tile at T = SEG, 2 SEG, 4 SEG, then the multi-tile T (the last entry of Ts)."""
    Ls = REG_WIDTHS[width]
    out = [Case(f"reg{width}_L{L}_B{B}_T{T}", REG, width, L, False, T, B, **kw) for L, T in zip(Ls, Ts)]
    out.append(Case(f"reg{width}_tiles_B{B}_T{Ts[-1]}", REG, width, Ls[-1], True, Ts[-1], B, **kw))
    return out


CASES = (
    _reg(4, 12, (64, 128, 256, 257)) + _reg(4, 2044, (64, 128, 256, 257)) + _reg(8, 2052, (32, 64, 128, 129)) +
    _reg(32, 16384, (8, 16, 32, 33)) + _reg(64, 98304, (4, 8, 16, 17)) + _reg(128, 393216, (2, 4, 5)) +
    _reg(256, 786432, (1, 2, 5)) + [
        # V-trace through every width's multi-tile instantiation
        Case("reg4_vtrace_B12_T257", REG, 4, 4, True, 257, 12, vtrace=True),
        Case("reg8_vtrace_B2052_T129", REG, 8, 4, True, 129, 2052, vtrace=True),
        Case("reg32_vtrace_B16384_T33", REG, 32, 4, True, 33, 16384, vtrace=True),
        Case("reg64_vtrace_B98304_T17", REG, 64, 4, True, 17, 98304, vtrace=True),
        Case("reg128_vtrace_B393216_T5", REG, 128, 2, True, 5, 393216, vtrace=True),
        Case("reg256_vtrace_B786432_T5", REG, 256, 2, True, 5, 786432, vtrace=True),
        Case("reg4_gl2_B2044_T257", REG, 4, 4, True, 257, 2044, gl=(0.9, 0.5)),
        Case("reg4_free_B12_T257", REG, 4, 4, True, 257, 12, free_flags=True),
        # LDS kernel, 16 columns per workgroup: one tile up to its budget, then two
        Case("lds16_plain_B37_T40", LDS, 16, 0, False, 40, 37),
        Case("lds16_plain_B5_T356", LDS, 16, 0, False, 356, 5),
        Case("lds16_plain_B37_T357", LDS, 16, 0, True, 357, 37),
        Case("lds16_gl2_B37_T357", LDS, 16, 0, True, 357, 37, gl=(0.9, 0.5)),
        Case("lds16_free_B37_T357", LDS, 16, 0, True, 357, 37, free_flags=True),
        Case("lds16_vtrace_B37_T255", LDS, 16, 0, True, 255, 37, vtrace=True),
        Case("lds16_both_B37_T163", LDS, 16, 0, True, 163, 37, vtrace=True, gamma_t=True, lambda_t=True),
        Case("lds16_gamma_B37_T163", LDS, 16, 0, False, 163, 37, gamma_t=True),
        Case("lds16_lambda_B37_T163", LDS, 16, 0, False, 163, 37, lambda_t=True),
        Case("lds16_gamma_B37_T199", LDS, 16, 0, True, 199, 37, gamma_t=True),
        Case("lds16_lambda_B37_T199", LDS, 16, 0, True, 199, 37, lambda_t=True),
        Case("lds16_nc3_B11_T357", LDS, 16, 0, True, 357, 11, Nc=3),
        Case("lds16_quadlayout_gamma_B12_T199", LDS, 16, 0, True, 199, 12, gamma_t=True),
        # LDS kernel, 64 columns per workgroup
        Case("lds64_plain_B32769_T89", LDS, 64, 0, True, 89, 32769),
        Case("lds64_vtrace_B32769_T89", LDS, 64, 0, True, 89, 32769, vtrace=True),
        Case("lds64_nc2_B16385_T20", LDS, 64, 0, False, 20, 16385, Nc=2),
        # shapes of the register kernel on a misaligned leaf: the LDS kernel takes them
        Case("misaligned_value_B12_T64", LDS, 16, 0, False, 64, 12, misalign="value"),
        Case("misaligned_done_B12_T64", LDS, 16, 0, False, 64, 12, misalign="done"),
        Case("misaligned_value_B16384_T8", LDS, 16, 0, False, 8, 16384, misalign="value"),
        Case("misaligned_done_B16384_T8", LDS, 16, 0, False, 8, 16384, misalign="done"),
        # degenerate
        Case("reg4_T1_B12", REG, 4, 1, False, 1, 12),
        Case("lds16_T1_B5", LDS, 16, 0, False, 1, 5),
        Case("reg4_onequad_B4_T7", REG, 4, 1, False, 7, 4),
    ])
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def plan_of(case: Case) -> dict:
    return hip.gae_scan_plan(case.T, case.B, case.Nc, aligned=case.misalign is None, vtrace=case.vtrace, tensors=case.tensors)


def assert_on_branch(case, plan):
    """The case runs the branch it names."""
    assert (plan["kernel"], plan["width"], plan["L"]) == (case.kernel, case.width, case.L), (case.name, plan)
    assert (plan["tiles"] > 1) == case.multi, (case.name, plan)
    assert plan["tiles"] == -(-case.T // plan["TT"]) and plan["grid"] == -(-case.B * case.Nc // (plan["width"] * (4 if case.kernel == REG else 1)))
    if case.kernel == REG:
        assert plan["TT"] == seg_of(plan) * plan["L"]
        if case.multi:
            assert case.T % plan["TT"] != 0, (case.name, plan)   # the tile holding row 0 is partial
    if case.misalign:
        aligned = hip.gae_scan_plan(case.T, case.B, case.Nc, vtrace=case.vtrace, tensors=case.tensors)
        assert aligned["kernel"] == REG and plan["kernel"] == LDS   # a register-kernel shape that the pointer test turns away


def seg_of(plan) -> int:
    """Chunks per column of a time tile: lanes along T."""
    return 256 // plan["width"]


def tile_starts(T, plan):
    """t0 of every time tile, in the order the kernels take them (from the end)."""
    return [max(t1 - plan["TT"], 0) for t1 in range(T, 0, -plan["TT"])]


def chunk_rows(T, plan) -> int:
    """Rows of a chunk in the first tile the kernels take (the one ending at T)."""
    n = T - tile_starts(T, plan)[0]
    return plan["L"] if plan["kernel"] == REG else -(-n // seg_of(plan))


def seam_rows(T, plan):
    """The rows the overlay puts every flag on: both sides of every tile seam, both sides of the first chunk seam of the tile
    ending at T (where there is one), row 0, row T - 1, the bootstrap row T."""
    rows = {0, T - 1, T}
    for t0 in tile_starts(T, plan):
        if t0 > 0:
            rows |= {t0 - 1, t0}
    seam = tile_starts(T, plan)[0] + chunk_rows(T, plan)
    if seam < T:
        rows |= {seam - 1, seam}
    return sorted(rows)


def quad_patterns(done, truncated, on_reset, row):
    """Per quad of adjacent columns, how many different (done, truncated, on_reset) patterns its four columns carry on `row`."""
    B = done.shape[1]
    code = (done[row, :B // 4 * 4, 0].astype(int) + 2 * truncated[row, :B // 4 * 4, 0] + 4 * on_reset[row, :B // 4 * 4, 0]).reshape(-1, 4)
    return np.array([len(set(q)) for q in code])


def build(case: Case, plan=None) -> dict:
    """The inputs of a case, numpy: reward [T+1, B, Nc] (row T unused), value [T+1, B, Nc], the flags [T+1, B, 1] uint8, ratio
    [T, B, 1] or None, gamma / lmbda (floats or [T, B, 1] float32), rho, c, and `rows`, the overlay's rows."""
    plan = plan_of(case) if plan is None else plan
    T, B, Nc = case.T, case.B, case.Nc
    assert B >= 3
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(case.name.encode())))
    rows = seam_rows(T, plan)
    if case.free_flags:
        done, truncated, on_reset = ((rng.random((T + 1, B, 1)) < 0.1).astype(np.uint8) for _ in range(3))
    else:
        done, truncated, on_reset = synthetic.make_flags(rng, T + 1, B, 0.03)
        quads = max(B // 4, 1)
        for i, r in enumerate(rows):   # done in column c0, truncated in c0 + 1, on_reset in c0 + 2 (it follows done[r - 1])
            c0 = 4 * (i % quads)
            cd, ct, co = c0 % B, (c0 + 1) % B, (c0 + 2) % B
            done[r, cd], truncated[r, cd] = 1, 0
            truncated[r, ct], done[r, ct] = 1, 0
            if r > 0:
                done[r - 1, co], truncated[r - 1, co] = 1, 0
        first = np.zeros((B, 1), np.uint8)
        first[2 % B] = 1                # row 0 has no predecessor: on_reset there is free
        on_reset = np.concatenate([first[None], done[:-1] | truncated[:-1]], axis=0)
    value = rng.standard_normal((T + 1, B, Nc)).astype(np.float32)
    value[value == 0] = 1.0
    reward = rng.standard_normal((T + 1, B, Nc)).astype(np.float32)
    reward[:-1] *= (1 - on_reset[1:])
    out = dict(reward=reward, value=value, done=done, truncated=truncated, on_reset=on_reset, ratio=None, gamma=case.gl[0],
               lmbda=case.gl[1], rho=1.0, c=1.0, rows=rows)
    if case.vtrace:
        out.update(ratio=rng.uniform(0.3, 1.8, size=(T, B, 1)).astype(np.float32), rho=RHO, c=C)
    if case.gamma_t:
        out["gamma"] = np.minimum(rng.uniform(0.9, 1.0, size=(T, B, 1)).astype(np.float32), np.nextafter(np.float32(1), np.float32(0)))
    if case.lambda_t:
        out["lmbda"] = np.minimum(rng.uniform(0.9, 1.0, size=(T, B, 1)).astype(np.float32), np.nextafter(np.float32(1), np.float32(0)))
    return out


def check_inputs(case: Case, a: dict):
    """What the inputs of a case promise: a non-zero value on done rows; for the overlaid cases every flag on every seam row, one
    quad with four different flag patterns on a row, and the reference's invariants."""
    done, truncated, on_reset = a["done"], a["truncated"], a["on_reset"]
    assert done.any() and (a["value"][np.broadcast_to(done == 1, a["value"].shape)] != 0).all()
    if case.free_flags:
        assert (truncated & on_reset).any() and (done & truncated).any()   # what make_flags forbids does occur
        return
    from oracle.gae import check_invariants
    check_invariants(a["reward"][:-1].astype(np.float64), a["value"], truncated.astype(np.float64), done.astype(np.float64),
                     on_reset.astype(np.float64))
    for r in a["rows"]:
        assert done[r].any() and truncated[r].any() and on_reset[r].any(), (case.name, r)
    if case.B >= 4:
        assert max(quad_patterns(done, truncated, on_reset, r).max() for r in a["rows"]) == 4, case.name
    if case.vtrace:
        q = a["ratio"]
        assert (q < C).any() and ((q > C) & (q < RHO)).any() and (q > RHO).any()


def reference(a, **kw):
    """`gae_ref.gae` on the inputs `build` returns."""
    return gae_ref.gae(a["reward"], a["value"], a["done"], a["truncated"], a["on_reset"], a["gamma"], a["lmbda"], ratio=a["ratio"],
                       rho=a["rho"], c=a["c"], **kw)
