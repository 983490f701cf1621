"""The image-stationary convolution kernel (`h2conv_kernel`, csrc/h2conv.h: conv2 / conv3 forward, conv3 / conv2 data gradient)
at the edges of its hand-written software pipeline.

Inside a batch of G images (G = 1 for conv2 forward, 2 for the others) the kernel runs its blocks of 16 positions as one
pinned instruction stream: the position fragments of k-block i + D are read between the MFMAs of k-block i through a ring of
register sets that runs on into the NEXT block, the previous block's epilogue (scale, bias, clamp, mask, amax, split, stores)
sits in pieces in the chain, and only a batch's first block opens with a burst of reads behind the batch's barrier.  The
batches of a workgroup rotate through a ring of 3 (forward) / 2 (data gradient) LDS slots; the grid is min(batches, 256).
What can go wrong is a fragment taken from the wrong slot, block or image, a read in front of its barrier, an epilogue that
meets the wrong accumulators, and a workgroup that takes one batch more than its neighbours.  So:

  * image counts around the ring depths and the grid: conv2 forward 1, 2, 3, 4, 257 (workgroup 0 takes a second batch), 259
    (three workgroups do), 769 (workgroup 0 takes a fourth batch: its three slots wrap); the others 1 .. 5, 513 (257 batches,
    the last half empty), 517, 1027 (workgroup 0 takes a third batch through its 2 or 3 slots, with an odd tail);
  * one different image B among copies of an image A, at the positions 0, 1, last, 256, 512 and 513: every output image must
    be, bit for bit, image 0 or image 1 of the two-image launch [A, B] (same bound and scale slots);
  * data gradients: dz non-zero only in the last row and the last column (the blocks whose tap rows are skipped, and the dense
    enumeration's last, partial block);
  * data gradients: all-zero mask bits in one image among three -- its dx is exactly zero, its neighbours' unchanged to the bit.

Reference: float64 torch `conv2d` / `conv_transpose2d` of the UNPACKED operands (`srl_h2_conv` through the C ABI; activations
packed with `srl_h2_pack_image` / `srl_h2_pack_rows` and read back with `srl_h2_unpack_image` / `srl_h2_unpack_rows`; the
weights are multiples of 2^-14 below 0.05 in magnitude, which both f16 pieces hold exactly -- checked for the forward layout,
whose rows `srl_h2_unpack_rows` reads back).  Tolerance: the one tests/test_gpu_h2.py holds these four launches to, 2e-6 of
the tensor's largest magnitude; sign bytes may differ from the reference's in at most 2 places (values at rounding distance
of zero), as there.  Compared: results, scales, out_absmax, mask bytes.  Every case's operands, packed buffers, reference and
first result are computed once and shared; each test prints a checksum of the bits it looked at."""
import functools
import hashlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 2e-6   # tests/test_gpu_h2.py::test_conv_forward_vs_float64 / test_conv_data_gradient_vs_float64
KINDS = ["f2", "f3", "d3", "d2"]
# layer geometry: H, Cin, k, stride, OH of the forward layer
GEO = dict(f2=(20, 32, 4, 2, 9), f3=(9, 64, 3, 1, 7), d3=(9, 64, 3, 1, 7), d2=(20, 32, 4, 2, 9))
COUNTS = dict(f2=[1, 2, 3, 4, 257, 259, 769], f3=[1, 2, 3, 4, 5, 513, 517, 1027], d3=[1, 2, 3, 4, 5, 513, 517, 1027],
              d2=[1, 2, 3, 4, 5, 513, 517, 1027])
HOT_N = dict(f2=769, f3=1027, d3=1027, d2=1027)
HOT = ["0", "1", "last", "256", "512", "513"]


def _hip():
    from srl_amd import hip
    hip.require_gpu()
    return hip


def _f(*shape, seed, relu=False, amp=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.rand(*shape, device=DEV, generator=g) * 2 - 1) * amp
    return torch.where(x < 0, torch.zeros_like(x), x * x * 3) if relu else x


def _slot():
    return torch.zeros(1, dtype=torch.float32, device=DEV)


def _absmax(hip, x):
    s = _slot()
    hip.absmax(x.data_ptr(), x.numel(), s.data_ptr())
    return s


def _pack_image(hip, x, layout):
    n, H, W, C = x.shape
    buf, scale, amax = torch.empty(x.numel(), dtype=torch.float32, device=DEV), _slot(), _absmax(hip, x)
    hip.h2_pack_image(x.data_ptr(), n, H, W, C, layout, buf.data_ptr(), absmax=amax.data_ptr(), scale_out=scale.data_ptr())
    return buf, scale, amax


def _pack_rows(hip, x, rows, cols):
    buf, scale, amax = torch.empty(x.numel(), dtype=torch.float32, device=DEV), _slot(), _absmax(hip, x)
    hip.h2_pack_rows(x.data_ptr(), cols, rows, cols, buf.data_ptr(), absmax=amax.data_ptr(), scale_out=scale.data_ptr())
    return buf, scale, amax


def _unpack_rows(hip, buf, scale, rows, cols):
    out = torch.empty(rows, cols, device=DEV)
    hip.h2_unpack_rows(buf.data_ptr(), rows, cols, scale.data_ptr(), out.data_ptr(), cols)
    return out


def _unpack_image(hip, buf, scale, n, H, C, layout):
    """NHWC float32 of a packed image; layout 2 (parity-class-major h2p rows) as rows, its pixels put back into raster order"""
    if layout == 0:
        out = torch.empty(n, H, H, C, device=DEV)
        hip.h2_unpack_image(buf.data_ptr(), n, H, H, C, 0, scale.data_ptr(), out.data_ptr())
        return out
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(H, device=DEV), indexing="ij")
    ent = (((yy & 1) * 2 + (xx & 1)) * (H // 2) * (H // 2) + (yy >> 1) * (H // 2) + (xx >> 1)).reshape(-1)
    return _unpack_rows(hip, buf, scale, n * H * H, C).view(n, H * H, C)[:, ent].reshape(n, H, H, C).contiguous()


def _mask_h2(act_nhwc):
    """Sign bytes in h2 order of a [n, H, W, C] activation: byte (pixel, block, group), bit j = element j of the group."""
    n, H, W, C = act_nhwc.shape
    a = (act_nhwc > 0).reshape(n * H * W, C // 32, 32)
    idx = torch.tensor([[4 * (g >> 1) + 16 * (g & 1) + (j & 3) + 8 * (j >> 2) for j in range(8)] for g in range(4)], device=DEV)
    w = (2 ** torch.arange(8, device=DEV)).to(torch.int32)
    return (a[:, :, idx].to(torch.int32) * w).sum(-1).to(torch.uint8).contiguous()


def _mask_natural(act_nhwc):
    a = (act_nhwc > 0).reshape(-1, 32).to(torch.int64)
    v = (a * 2 ** torch.arange(32, device=DEV, dtype=torch.int64)).sum(-1)
    return torch.where(v >= 2**31, v - 2**32, v).to(torch.int32).contiguous()


@functools.lru_cache(maxsize=None)
def _layer(kind):
    """Weights (multiples of 2^-14: exact in the packed format) and bias of the layer, and the packed weights of the launch."""
    hip = _hip()
    H, C, k, st, OH = GEO[kind]
    w = torch.round(_f(64, k, k, C, seed=4 if kind[0] == "f" else 7, amp=0.05) * 2**14) / 2**14   # [Cout, KH, KW, Cin]
    b = _f(64, seed=5, amp=0.1)
    amax, s, r = _absmax(hip, w), _slot(), _slot()
    if kind[0] == "f":
        rows, K, mode, desc = 64, k * k * C, 0, None
    else:
        rows, K, mode, desc = st * st * C, (k // st) * (k // st) * 64, 2, hip.conv_desc(1, H, H, C, k, k, st, 64, 1)
    wp = torch.empty(rows * K, dtype=torch.float32, device=DEV)
    hip.h2_weights(w.data_ptr(), rows, K, mode, amax.data_ptr(), s.data_ptr(), r.data_ptr(), wp.data_ptr(), desc=desc)
    if kind[0] == "f":
        assert torch.equal(_unpack_rows(hip, wp, s, rows, K), w.reshape(rows, K))
    return w, b, wp, s, r, _absmax(hip, b)


class Case:
    """Operands of one launch, packed; `run()` launches and returns (result buffer, mask bytes or None, scale, absmax)."""

    def __init__(self, kind, src, act=None):
        """src: the forward kernels' input activation / the data gradients' dz (NHWC float32); act: data gradients: the forward
        activation whose ReLU derivative gates dx"""
        hip = _hip()
        H, C, k, st, OH = GEO[kind]
        self.hip, self.kind, self.n = hip, kind, src.shape[0]
        self.w, self.b, self.wp, self.sw, self.rw, self.bb = _layer(kind)
        if kind == "f2":
            self.buf, self.sx, self.ax = _pack_image(hip, src, 2)
            self.src = _unpack_image(hip, self.buf, self.sx, self.n, H, C, 2)
        elif kind == "d3":
            self.buf, self.sx, self.ax = _pack_rows(hip, src, self.n * OH * OH, 64)
            self.src = _unpack_rows(hip, self.buf, self.sx, self.n * OH * OH, 64).view(self.n, OH, OH, 64)
        else:
            HH, CC = (H, C) if kind == "f3" else (OH, 64)
            self.buf, self.sx, self.ax = _pack_image(hip, src, 0)
            self.src = _unpack_image(hip, self.buf, self.sx, self.n, HH, CC, 0)
        assert float((self.src - src).abs().max()) <= 2.0**-21 * float(src.abs().max())
        self.act = act
        self.mask_in = None if act is None else (_mask_h2(act) if kind == "d3" else _mask_natural(act))
        self.code = dict(f2=hip.H2_CONV2_FWD, f3=hip.H2_CONV3_FWD, d3=hip.H2_CONV3_DGRAD, d2=hip.H2_CONV2_DGRAD)[kind]
        self.out_shape = (self.n, OH, OH, 64) if kind[0] == "f" else (self.n, H, H, C)

    def run(self, mask_in=None):
        hip, n = self.hip, self.n
        out = torch.zeros(self.out_shape, device=DEV).reshape(-1)
        osc, oam = _slot(), _slot()
        if self.kind[0] == "f":
            mask = torch.zeros(out.numel() // 8, dtype=torch.uint8, device=DEV)
            hip.h2_conv(self.code, self.buf.data_ptr(), self.wp.data_ptr(), self.sx.data_ptr(), self.sw.data_ptr(), n, out.data_ptr(),
                        oam.data_ptr(), bias=self.b.data_ptr(), act=1, out_scale=osc.data_ptr(), bound_in=self.ax.data_ptr(),
                        bound_w=self.rw.data_ptr(), bound_b=self.bb.data_ptr(), mask_out=mask.data_ptr())
        else:
            mask = None
            mi = self.mask_in if mask_in is None else mask_in
            hip.h2_conv(self.code, self.buf.data_ptr(), self.wp.data_ptr(), self.sx.data_ptr(), self.sw.data_ptr(), n, out.data_ptr(),
                        oam.data_ptr(), out_scale=osc.data_ptr(), bound_in=self.ax.data_ptr(), bound_w=self.rw.data_ptr(),
                        mask_in=mi.data_ptr())
        return out, mask, osc, oam

    @functools.cached_property
    def first(self):
        return self.run()

    def unpacked(self, res):
        """NHWC float32 of a result"""
        out, mask, osc, oam = res
        n, OH = self.n, GEO[self.kind][4]
        if self.kind == "f2":
            return _unpack_image(self.hip, out, osc, n, OH, 64, 0)
        if self.kind == "f3":
            return _unpack_rows(self.hip, out, osc, n * OH * OH, 64).view(n, OH, OH, 64)
        if self.kind == "d3":
            return _unpack_image(self.hip, out, osc, n, 9, 64, 0)
        return out.view(self.out_shape)

    @functools.cached_property
    def ref(self):
        """float64 NHWC result of the unpacked operands"""
        st = GEO[self.kind][3]
        wd = self.w.double().permute(0, 3, 1, 2)
        if self.kind[0] == "f":
            return F.relu(F.conv2d(self.src.double().permute(0, 3, 1, 2), wd, self.b.double(), stride=st)).permute(0, 2, 3, 1).contiguous()
        return (F.conv_transpose2d(self.src.double().permute(0, 3, 1, 2), wd, stride=st).permute(0, 2, 3, 1) * (self.act > 0)).contiguous()

    def check(self, res):
        """result against float64 at TOL; the scale is a power of two that keeps the range in f16; out_absmax is the range; the
        forward kernels' sign bytes are the signs"""
        out, mask, osc, oam = res
        got, ref = self.unpacked(res), self.ref
        err, top = float((got.double() - ref).abs().max()), max(float(ref.abs().max()), 1e-30)
        print(f"{self.kind} n={self.n}: max error {err:.3e} of {top:.3e}: {err / top:.3e} (bound {TOL:.0e})")
        assert err <= TOL * top, (err, top)
        gtop = float(got.abs().max())
        assert abs(float(oam) - gtop) <= 1e-5 * gtop and top <= gtop * (1 + 1e-5)
        if self.kind != "d2":
            sc = float(osc)
            assert sc > 0 and torch.frexp(osc)[0].item() == 0.5 and gtop * sc < 2**15
        if mask is not None:
            assert int((mask.view(-1) != _mask_h2(ref.float()).view(-1)).sum()) <= 2


def _same(r1, r2):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(r1, r2))


def _checksum(tag, res):
    h = hashlib.sha1()
    for t in res:
        if t is not None:
            h.update(t.cpu().numpy().tobytes())
    print(f"checksum {tag} {h.hexdigest()}")


def _operands(kind, n, seed=0):
    H, C, k, st, OH = GEO[kind]
    if kind[0] == "f":
        return _f(n, H, H, C, seed=3 + seed, relu=True, amp=2.0), None
    return _f(n, OH, OH, 64, seed=6 + seed, amp=1e-3), _f(n, H, H, C, seed=8 + seed, relu=True)


@functools.lru_cache(maxsize=None)
def _dense(kind, n):
    return Case(kind, *_operands(kind, n))


def _pos(kind, pos):
    return HOT_N[kind] - 1 if pos == "last" else int(pos)


@functools.lru_cache(maxsize=None)
def _pair(kind):
    """the two-image launch [A, B]"""
    (a, aa), (b, ab) = _operands(kind, 1, seed=100), _operands(kind, 1, seed=200)
    return Case(kind, torch.cat([a, b]), None if aa is None else torch.cat([aa, ab]))


@functools.lru_cache(maxsize=None)
def _one_different(kind, pos):
    """HOT_N images, all copies of A but image `pos`, which is B"""
    (a, aa), (b, ab) = _operands(kind, 1, seed=100), _operands(kind, 1, seed=200)
    n, i = HOT_N[kind], _pos(kind, pos)
    src = a.repeat(n, 1, 1, 1)
    src[i] = b[0]
    act = None
    if aa is not None:
        act = aa.repeat(n, 1, 1, 1)
        act[i] = ab[0]
    return Case(kind, src, act)


@functools.lru_cache(maxsize=None)
def _last_row_col(kind):
    dz, act = _operands(kind, 3)
    keep = torch.zeros_like(dz)
    keep[:, -1, :, :] = 1
    keep[:, :, -1, :] = 1
    return Case(kind, dz * keep, act)


@pytest.mark.parametrize("kind,n", [(k, n) for k in KINDS for n in COUNTS[k]])
def test_image_counts_vs_float64(kind, n):
    case = _dense(kind, n)
    case.check(case.first)
    _checksum(f"counts {kind} {n}", case.first)


@pytest.mark.parametrize("kind,n", [(k, n) for k in KINDS for n in COUNTS[k]])
def test_two_further_calls_same_bits(kind, n):
    case = _dense(kind, n)
    for _ in range(2):
        assert _same(case.run(), case.first)


@pytest.mark.parametrize("pos", HOT)
@pytest.mark.parametrize("kind", KINDS)
def test_one_different_image(kind, pos):
    """Image 0, 1: the first batch of a workgroup; 256: workgroup 128's second batch (conv2 forward: workgroup 0's); 512, 513:
    the first batch workgroup 0 takes a second time round (conv2 forward: its third, the ring's last slot); last: the tail.
    A fragment from another slot, block or image, or one read before its barrier, meets the other image's values.  The bound and
    scale slots are those of the two-image launch [A, B] (same largest magnitudes), so every output image -- values, and the
    forward kernels' sign bytes -- is one of that launch's two, bit for bit."""
    case, pair = _one_different(kind, pos), _pair(kind)
    assert torch.equal(case.sx, pair.sx) and torch.equal(case.ax, pair.ax)
    (out, mask, osc, oam), (pout, pmask, posc, poam) = case.first, pair.first
    assert torch.equal(osc, posc) and torch.equal(oam, poam)
    n, i = case.n, _pos(kind, pos)
    want = torch.zeros(n, dtype=torch.long, device=DEV)
    want[i] = 1
    assert torch.equal(out.view(n, -1), pout.view(2, -1)[want])
    if mask is not None:
        assert torch.equal(mask.view(n, -1), pmask.view(2, -1)[want])
    pair.check(pair.first)
    _checksum(f"one-different {kind} {pos}", case.first)


@pytest.mark.parametrize("kind", ["d3", "d2"])
def test_dz_in_last_row_and_column_only(kind):
    """dz's last row and column reach the outputs' last rows and columns only through some taps: these are the blocks whose
    tap rows are skipped, and the dense enumeration's last, partial block -- a fragment of a neighbouring block or tap meets
    zeros."""
    case = _last_row_col(kind)
    case.check(case.first)
    assert _same(case.run(), case.first)
    _checksum(f"last-row-col {kind}", case.first)


@pytest.mark.parametrize("kind", ["d3", "d2"])
def test_all_zero_mask_in_one_image_among_three(kind):
    """The ReLU-derivative bits ride in with their batch: image 1's all-zero bits must zero image 1's dx and nothing else."""
    case = _dense(kind, 3)
    act = case.act.clone()
    act[1] = 0
    res = case.run(mask_in=_mask_h2(act) if kind == "d3" else _mask_natural(act))
    out, ref = res[0].view(3, -1), case.first[0].view(3, -1)
    assert int((out[1].view(torch.int32) != 0).sum()) == 0
    assert torch.equal(out[0], ref[0]) and torch.equal(out[2], ref[2])
    _checksum(f"zero-mask {kind}", res)
