"""Which kernel family takes a dense product or an NHWC convolution: ``srl_gemm_family`` / ``srl_conv2d_family`` (the rule the
entry points themselves branch on) against a literal table with one row per branch edge, under the A/B switches the library
reads per call.  The table's default column is what the library's launches counted (``dispatch_tiles``) before the queries
existed; the GPU test at the end holds the launches to it.  The host tests need the built library, not a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from srl_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, F, X, M, T = hip.FAMILY_SKINNY, hip.FAMILY_F32, hip.FAMILY_X3, hip.FAMILY_X3_SMALL, hip.FAMILY_TWO
SWITCHES = ("SRL_MFMA", "SRL_F16X2", "SRL_SMALL_GEMM", "SRL_OBS_BF16")
# the columns of `want` below: default, SRL_MFMA=f32, SRL_F16X2=0, SRL_SMALL_GEMM=0
SETTINGS = ({}, {"SRL_MFMA": "f32"}, {"SRL_F16X2": "0"}, {"SRL_SMALL_GEMM": "0"})

# (id, (M, N, K), descriptor fields beyond the plain forward orientation, ranges known?, want per setting)
GEMM_ROWS = [
    ("skinny", (16, 64, 256), dict(a_kmajor=1, b_kmajor=1, accumulate=1), False, (S, S, S, S)),  # one extent <= 16 (a head's weight gradient)
    ("small_m64", (64, 65, 64), {}, False, (M, F, M, F)),            # M <= 64 -- but few outputs and K <= 512: 64 x 64 tiles first
    ("f32_m64", (64, 65, 516), {}, True, (F, F, F, F)),              # M <= 64 and K > 512
    ("small", (256, 256, 128), {}, False, (M, F, M, X)),             # <= 65 536 outputs
    ("small_ranges", (256, 256, 128), {}, True, (M, F, M, T)),       # ... whatever the ranges
    ("two_outputs", (257, 256, 64), {}, True, (T, F, X, T)),         # > 65 536 outputs
    ("two_k", (65, 65, 516), {}, True, (T, F, X, T)),                # K > 512
    ("x3_outputs", (257, 256, 64), {}, False, (X, F, X, X)),         # ranges missing
    ("x3_k", (65, 65, 516), {}, False, (X, F, X, X)),
    ("x3_n64", (257, 64, 516), {}, True, (X, F, X, X)),              # 32 < N <= 64: no two-piece 256 x 64 tile
    ("f32_lda", (257, 256, 64), dict(lda=65), True, (F, F, F, F)),   # lda = K + 1: not float4-stageable
    ("f32_akm", (258, 256, 64), dict(a_kmajor=1), True, (F, F, F, F)),  # k-major A, M % 4 != 0
]

FWD, DGRAD, WGRAD = hip.PASS_FWD, hip.PASS_DGRAD, hip.PASS_WGRAD
# (id, pass, (H = W, Cin, k, stride, Cout), ranges known?, want for default / SRL_MFMA=f32 / SRL_F16X2=0); SRL_SMALL_GEMM=0 as default
CONV_ROWS = [
    ("fwd_c64", FWD, (12, 32, 3, 1, 64), True, (T, F, X)),
    ("fwd_c96", FWD, (12, 32, 3, 1, 96), True, (T, F, X)),
    ("fwd_c64_noranges", FWD, (12, 32, 3, 1, 64), False, (X, F, X)),
    ("fwd_c32", FWD, (12, 32, 3, 1, 32), True, (F, F, F)),
    ("fwd_kp36", FWD, (12, 4, 3, 1, 64), True, (F, F, F)),            # Kp = 36 < 64
    ("wgrad_c64", WGRAD, (12, 32, 3, 1, 64), True, (T, F, X)),
    ("wgrad_c64_noranges", WGRAD, (12, 32, 3, 1, 64), False, (X, F, X)),
    ("wgrad_c32", WGRAD, (12, 32, 3, 1, 32), True, (F, F, F)),
    ("dgrad_strided", DGRAD, (20, 32, 4, 2, 64), True, (T, F, X)),    # test_presplit_weights_give_the_same_bits' two geometries:
    ("dgrad_stride1", DGRAD, (9, 64, 3, 1, 64), True, (T, F, X)),     # four classes packed to 128 columns; one class of 64
    ("dgrad_odd", DGRAD, (21, 64, 4, 2, 64), True, (T, F, X)),        # odd H: the classes' row grids differ, one product each
    ("dgrad_noranges", DGRAD, (9, 64, 3, 1, 64), False, (X, F, X)),
    ("dgrad_c24", DGRAD, (9, 64, 3, 1, 24), True, (F, F, F)),         # Cout % 16 != 0: a k-step would straddle two taps
    ("dgrad_cols32", DGRAD, (9, 32, 3, 1, 64), True, (F, F, F)),      # 32 columns
    ("dgrad_odd_cols32", DGRAD, (21, 32, 4, 2, 64), True, (F, F, F)), # not packed: Cin columns per class
]


def gemm_desc(shape, extra, ranges, ptr=lambda name, floats: 0x10000):
    """The row's descriptor; `ptr(name, floats)` supplies the addresses (the query reads their alignment only)."""
    m, n, k = shape
    akm, bkm = extra.get("a_kmajor", 0), extra.get("b_kmajor", 0)
    lda, ldb = extra.get("lda", m if akm else k), n if bkm else k
    d = hip.GemmDesc(M=m, N=n, K=k, lda=lda, a_kmajor=akm, ldb=ldb, b_kmajor=bkm, ldc=n, accumulate=extra.get("accumulate", 0))
    d.A, d.B, d.C = ptr("A", (k if akm else m) * lda), ptr("B", (k if bkm else n) * ldb), ptr("C", m * n)
    if ranges:
        d.a_absmax, d.b_absmax = ptr("a_absmax", 1), ptr("b_absmax", 1)
    return d


def conv_desc(geom, n=8):
    h, cin, k, s, cout = geom
    return hip.conv_desc(n, h, h, cin, k, k, s, cout)


def _set(monkeypatch, setting):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in SETTINGS[setting].items():
        monkeypatch.setenv(name, value)


@pytest.mark.parametrize("setting", range(len(SETTINGS)), ids=["default", "mfma_f32", "f16x2_0", "small_gemm_0"])
def test_family_queries_match_the_table(monkeypatch, setting):
    _set(monkeypatch, setting)
    for name, shape, extra, ranges, want in GEMM_ROWS:
        d = gemm_desc(shape, extra, ranges)
        fam = hip.lib().srl_gemm_family(ctypes.byref(d))
        assert fam == want[setting], (name, fam)
        # the binding's query (it knows the orientations, not the epilogue: a skinny row is some other non-two-piece family to it)
        args = (*shape, d.A, d.lda, d.B, d.ldb, d.a_absmax, d.b_absmax)
        if fam != S:
            assert hip.gemm_family(*args, a_kmajor=d.a_kmajor, b_kmajor=d.b_kmajor) == fam, name
        assert hip.gemm_two_piece(*args, a_kmajor=d.a_kmajor, b_kmajor=d.b_kmajor) == (fam == T), name
    for name, pass_, geom, ranges, want in CONV_ROWS:
        d, r = conv_desc(geom), (1 if ranges else None)
        fam = hip.conv2d_family(d, pass_, ranges)
        assert fam == want[setting % 3], (name, fam)
        if pass_ == FWD:
            assert hip.conv2d_fwd_two_piece(d, r, r) == (fam == T), name
        if pass_ == DGRAD:
            assert hip.conv2d_dgrad_two_piece(d, r, r) == (fam == T), name
    assert hip.lib().srl_gemm_family(None) == -1
    assert hip.conv2d_family(hip.conv_desc(8, 12, 12, 30, 3, 3, 1, 64), FWD) == -1          # Cin % 4 != 0: the pass rejects it
    assert hip.conv2d_family(hip.conv_desc(8, 40, 40, 32, 9, 9, 9, 64), DGRAD, True) == -1  # stride > 8
    assert hip.conv2d_family(conv_desc((12, 32, 3, 1, 64)), 7) == -1


def test_first_layer_family_rests_on_the_byte_kernels_geometry(monkeypatch):
    """Byte frames, channels-last, Kp = 256, 32 output channels, >= 32 images: the bf16 byte kernels (X3); the backward with a bound of
    |dz| on the Atari geometry the two-piece block kernel; everything else, and SRL_OBS_BF16=0, float32 MFMA.  A batch walked in
    several runs is walked in EQUAL runs, so every size above the limit that keeps its runs at 32 images answers alike."""
    _set(monkeypatch, 0)
    atari = lambda n: hip.conv_desc(n, 21, 21, 64, 2, 2, 1, 32)
    q = lambda d, pass_, ranges=False, u8=True, cl=True: hip.conv2d_family(d, pass_, ranges, u8, cl)
    OF, OB = hip.PASS_OBS_FWD, hip.PASS_OBS_BWD
    assert q(atari(64), OF) == X and q(atari(64), OB) == X and q(atari(64), OB, True) == T
    assert q(atari(31), OF) == F and q(atari(31), OB, True) == F                      # fewer than 32 images
    assert q(atari(64), OF, u8=False) == F and q(atari(64), OB, True, u8=False) == F  # float32 frames
    other = hip.conv_desc(64, 11, 11, 32, 2, 4, 1, 32)                                # Kp = 256, not the block kernel's geometry
    assert q(other, OF) == X and q(other, OB, True) == X
    assert q(hip.conv_desc(64, 84, 84, 4, 8, 8, 4, 32), OF, u8=True, cl=False) == F   # planar frames
    monkeypatch.setenv("SRL_CONV_RUN_IMAGES", "40")
    assert [q(atari(n), OF) for n in (33, 41, 64, 100, 1000)] == [X, F, X, X, X]      # runs of 33 | 21, 20 | 32 x 2 | 34, 34, 32 | 40 x 25
    assert [q(atari(n), OB, True) for n in (33, 41, 64, 100, 1000)] == [T, F, T, T, T]
    monkeypatch.delenv("SRL_CONV_RUN_IMAGES")
    monkeypatch.setenv("SRL_OBS_BF16", "0")
    assert q(atari(64), OF) == F and q(atari(64), OB, True) == F


def test_python_reads_none_of_the_dispatch_switches():
    """The library owns the rule and the switches; the package asks it."""
    for base, _, files in os.walk(os.path.join(ROOT, "srl_amd")):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(base, f)).read()
                assert not re.search("|".join(SWITCHES), text), os.path.join(base, f)
    assert not hasattr(hip, "f16x2_enabled")
    assert [hip.piece_products(k) for k in ("f32", "x3", "2h", "obs", "obs2")] == [1.0, 6.0, 3.0, 3.0, 2.0]


# ------------------------------------------------------------------------------------------------ what the launches count
DEV = "cuda:0"


def _ran():
    """The families of the launches since the last reset, from the library's counters."""
    tiles, counts = hip.dispatch_tiles(reset=True), hip.dispatch_counts(reset=True)
    fams = {S} if counts["skinny"] else set()
    for label in tiles:
        name, tile = label.split(":")[:2]
        fams.add({"gemm2h": T, "gemm_f32": F, "gemm3": M if tile == "64x64" else X}[name])
    return fams


def _rand(rng, floats):
    return torch.from_numpy(rng.standard_normal(floats).astype(np.float32)).to(DEV)


def _presplit(t, absmax):
    out = torch.empty_like(t)
    hip.presplit(t.data_ptr(), absmax.data_ptr(), out.data_ptr(), t.numel())
    return out


@pytest.mark.gpu
def test_launches_run_the_family_the_query_names():
    """Every row at the library's default switches, launched: the counters show exactly the family the query named (and the table,
    unless the process runs under one of the switches); a pre-split B / w / wt is accepted iff that family is the two-piece one,
    then gives the same bits, and is otherwise refused as an argument error that names it, before any launch."""
    rng = np.random.default_rng(5)
    default_env = not any(name in os.environ for name in SWITCHES)
    _ran()
    for name, shape, extra, ranges, want in GEMM_ROWS:
        bufs = {}

        def ptr(which, floats):
            bufs[which] = _rand(rng, floats).abs_() if which.endswith("absmax") else _rand(rng, floats)
            return bufs[which].data_ptr()

        d = gemm_desc(shape, extra, ranges, ptr)
        if ranges:
            bufs["a_absmax"].copy_(bufs["A"].abs().max())
            bufs["b_absmax"].copy_(bufs["B"].abs().max())
        fam = hip.lib().srl_gemm_family(ctypes.byref(d))
        assert not default_env or fam == want[0], (name, fam)
        kw = dict(accumulate=bool(d.accumulate), a_absmax=d.a_absmax, b_absmax=d.b_absmax)
        c0 = bufs["C"].clone()
        hip.gemm(*shape, d.A, d.lda, d.a_kmajor, d.B, d.ldb, d.b_kmajor, d.C, d.ldc, **kw)
        assert _ran() == {fam}, name
        if fam == T:
            b2, c1 = _presplit(bufs["B"], bufs["b_absmax"]), c0.clone()
            hip.gemm(*shape, d.A, d.lda, d.a_kmajor, b2.data_ptr(), d.ldb, d.b_kmajor, c1.data_ptr(), d.ldc, b_presplit=True, **kw)
            assert torch.equal(c1, bufs["C"]) and _ran() == {T}, name
        else:
            with pytest.raises(hip.HipError, match="b_presplit"):
                hip.gemm(*shape, d.A, d.lda, d.a_kmajor, d.B, d.ldb, d.b_kmajor, d.C, d.ldc, b_presplit=True, **kw)
            assert _ran() == set(), name
    for name, pass_, geom, ranges, want in CONV_ROWS:
        d = conv_desc(geom)
        h, cin, k, s, cout = geom
        oh = (h - k) // s + 1
        x, w, dz = _rand(rng, (8, h, h, cin)), _rand(rng, (cout, k, k, cin)) / k, _rand(rng, (8, oh, oh, cout))
        r = (lambda t: t.abs().max().reshape(1)) if ranges else (lambda t: None)
        xr, wr, dzr = r(x), r(w), r(dz)
        p = lambda t: None if t is None else t.data_ptr()
        fam = hip.conv2d_family(d, pass_, ranges)
        assert not default_env or fam == want[0], (name, fam)
        if pass_ == WGRAD:
            dw = torch.zeros_like(w)
            ws = torch.empty(max(hip.conv2d_wgrad_workspace(d), 1), device=DEV)
            hip.conv2d_nhwc_wgrad(d, x.data_ptr(), dz.data_ptr(), dw.data_ptr(), ws.data_ptr(), x_absmax=p(xr), dz_absmax=p(dzr))
            assert _ran() == {fam}, name
            continue
        if pass_ == FWD:
            out = lambda: torch.full((8, oh, oh, cout), np.nan, device=DEV)
            run = lambda wt, y, **kw: hip.conv2d_nhwc_fwd(d, x.data_ptr(), wt.data_ptr(), None, y.data_ptr(), x_absmax=p(xr),
                                                          w_absmax=p(wr), **kw)
            arg = "w_presplit"
        else:
            wt = torch.empty(hip.conv2d_dgrad_weight_elems(d), device=DEV)
            hip.conv2d_dgrad_repack(d, w.data_ptr(), wt.data_ptr())
            w = wt
            out = lambda: torch.full((8, h, h, cin), np.nan, device=DEV)
            run = lambda wt, y, **kw: hip.conv2d_nhwc_dgrad(d, dz.data_ptr(), wt.data_ptr(), None, 0, y.data_ptr(), dz_absmax=p(dzr),
                                                            w_absmax=p(wr), **kw)
            arg = "wt_presplit"
        y0, y1 = out(), out()
        run(w, y0)
        assert _ran() == {fam}, name
        if fam == T:
            run(_presplit(w, wr), y1, presplit=True)
            assert torch.equal(y0, y1) and not torch.isnan(y0).any() and _ran() == {T}, name
        else:
            with pytest.raises(hip.HipError, match=arg):
                run(w, y1, presplit=True)
            assert _ran() == set(), name
