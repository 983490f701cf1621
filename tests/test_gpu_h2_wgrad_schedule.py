"""The convolution weight-gradient kernel (`h2wgrad_kernel`, csrc/h2conv.h) at the edges of its hand-written software pipeline.

Within an image the kernel fetches the fragments of step k + 1 between the MFMAs of step k and re-reads the dz fragments of the
next chunk into the registers of the current one; an image starts with a burst behind its barrier and ends without reads; the
images of a workgroup rotate through a ring of 2 (conv2) / 3 (conv3) LDS slots.  What can go wrong is a fragment taken from
the wrong slot, chunk or step, and a workgroup that finishes an iteration earlier than its neighbours.  So: image counts 1
(prologue and drain with nothing between), 2 and 3 (the ring depths), 4, and 259 -- three of the 256 workgroups take a second
image --; one non-zero image among 259 at the positions 0, 1, 256 and 258; dz non-zero in the last output row and column only.

Reference: float64 torch convolution weight / bias gradient of the UNPACKED h2 operands (`srl_h2_wgrad` through the C ABI; inputs
packed with `srl_h2_pack_image` / `srl_h2_pack_rows`, read back with `srl_h2_unpack_image` / `srl_h2_unpack_rows`).  Tolerance:
the one tests/test_gpu_h2.py holds these two launches to at batches of up to 2048 images -- 1e-6 of the tensor's largest
magnitude (two f16 pieces per operand: 2^-22 per product, float32 accumulation).  Every case's operands, packed buffers,
reference and first result are computed once and shared."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-6   # tests/test_gpu_h2.py::test_conv_weight_gradient_vs_float64, n <= 2048
GEO = dict(c2=(20, 32, 4, 2, 9), c3=(9, 64, 3, 1, 7))   # H, Cin, k, stride, OH
COUNTS = [1, 2, 3, 4, 259]
HOT = [0, 1, 256, 258]


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
    return buf, scale


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


def _pack_rows(hip, x, rows, cols):
    buf, scale, amax = torch.empty(x.numel(), dtype=torch.float32, device=DEV), _slot(), _absmax(hip, x)
    hip.h2_pack_rows(x.data_ptr(), cols, rows, cols, buf.data_ptr(), absmax=amax.data_ptr(), scale_out=scale.data_ptr())
    return buf, scale


class Case:
    """Operands of one launch, packed; `run(gw, gb)` adds the launch's gradients into the two buffers."""

    def __init__(self, kind, x, dz):
        hip = _hip()
        H, C, k, st, OH = GEO[kind]
        self.kind, self.n, self.K = kind, x.shape[0], k * k * C
        self.xbuf, self.sx = _pack_image(hip, x, 2 if kind == "c2" else 0)
        self.zbuf, self.sz = _pack_image(hip, dz, 0) if kind == "c2" else _pack_rows(hip, dz, self.n * OH * OH, 64)
        # what the kernel is given, as float32
        self.x = _unpack_image(hip, self.xbuf, self.sx, self.n, H, C, 2 if kind == "c2" else 0)
        self.dz = (_unpack_image(hip, self.zbuf, self.sz, self.n, OH, 64, 0) if kind == "c2"
                   else _unpack_rows(hip, self.zbuf, self.sz, self.n * OH * OH, 64).view(self.n, OH, OH, 64))
        assert float((self.x - x).abs().max()) <= 2.0**-21 * float(x.abs().max()) and float((self.dz - dz).abs().max()) <= 2.0**-21 * float(dz.abs().max())
        self.code = hip.H2_WGRAD_CONV2 if kind == "c2" else hip.H2_WGRAD_CONV3
        self.ws = torch.empty(hip.h2_wgrad_workspace(self.code), device=DEV)
        self.hip = hip

    def run(self, gw, gb):
        self.hip.h2_wgrad(self.code, self.xbuf.data_ptr(), self.zbuf.data_ptr(), self.sx.data_ptr(), self.sz.data_ptr(), self.n,
                          self.ws.data_ptr(), gw.data_ptr(), gb.data_ptr())
        return gw, gb

    def fresh(self):
        return self.run(torch.zeros(64, self.K, device=DEV), torch.zeros(64, device=DEV))

    @functools.cached_property
    def first(self):
        return self.fresh()

    @functools.cached_property
    def ref(self):
        """float64 (dW [64][tap][cin], db [64]) of the unpacked operands"""
        H, C, k, st, OH = GEO[self.kind]
        wd = torch.zeros(64, C, k, k, dtype=torch.float64, device=DEV, requires_grad=True)
        bd = torch.zeros(64, dtype=torch.float64, device=DEV, requires_grad=True)
        (F.conv2d(self.x.double().permute(0, 3, 1, 2), wd, bd, stride=st) * self.dz.double().permute(0, 3, 1, 2)).sum().backward()
        return wd.grad.permute(0, 2, 3, 1).reshape(64, self.K), bd.grad


def _operands(kind, n):
    H, C, k, st, OH = GEO[kind]
    return _f(n, H, H, C, seed=9, relu=True, amp=2.0), _f(n, OH, OH, 64, seed=10, amp=1e-3)


@functools.lru_cache(maxsize=None)
def _dense(kind, n):
    return Case(kind, *_operands(kind, n))


@functools.lru_cache(maxsize=None)
def _one_hot(kind, pos):
    """259 images, all zero but image `pos`, which is image 0 of the one-image case"""
    x1, dz1 = _operands(kind, 1)
    x, dz = torch.zeros(259, *x1.shape[1:], device=DEV), torch.zeros(259, *dz1.shape[1:], device=DEV)
    x[pos], dz[pos] = x1[0], dz1[0]
    return Case(kind, x, dz)


@functools.lru_cache(maxsize=None)
def _last_row_col(kind):
    x, dz = _operands(kind, 3)
    keep = torch.zeros_like(dz)
    keep[:, -1, :, :] = 1
    keep[:, :, -1, :] = 1
    return Case(kind, x, dz * keep)


def _close(got, ref):
    err = float((got.to(torch.float64) - ref).abs().max())
    top = max(float(ref.abs().max()), 1e-30)
    print(f"max error {err:.3e} of {top:.3e}: {err / top:.3e} (bound {TOL:.0e})")
    assert err <= TOL * top, (err, top)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", ["c2", "c3"])
def test_image_counts_vs_float64(kind, n):
    case = _dense(kind, n)
    (gw, gb), (rw, rb) = case.first, case.ref
    _close(gw, rw)
    _close(gb, rb)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", ["c2", "c3"])
def test_two_calls_same_bits(kind, n):
    case = _dense(kind, n)
    gw, gb = case.fresh()
    assert torch.equal(gw, case.first[0]) and torch.equal(gb, case.first[1])


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", ["c2", "c3"])
def test_second_call_doubles_to_the_bit(kind, n):
    """The launch ADDS into the gradient buffers: s + s is exact in float32."""
    case = _dense(kind, n)
    gw, gb = case.run(*case.fresh())
    assert torch.equal(gw, 2 * case.first[0]) and torch.equal(gb, 2 * case.first[1])


@pytest.mark.parametrize("pos", HOT)
@pytest.mark.parametrize("kind", ["c2", "c3"])
def test_one_nonzero_image_among_259(kind, pos):
    """Image 0, 1: a workgroup's only image; 256, 258: the second image of workgroups 0 and 2, in the slot and behind the
    barrier that follow a first image of zeros.  A fragment read from another slot or before its barrier reads zeros (or the
    slot's previous image).  The scales are those of the one-image case (same largest magnitudes) and a sum with exact zeros
    changes nothing: the result is also, bit for bit, the one-image launch's."""
    case, single = _one_hot(kind, pos), _dense(kind, 1)
    (gw, gb), (rw, rb) = case.first, single.ref
    _close(gw, rw)
    _close(gb, rb)
    assert torch.equal(gw, single.first[0]) and torch.equal(gb, single.first[1])


@pytest.mark.parametrize("kind", ["c2", "c3"])
def test_dz_in_last_row_and_column_only(kind):
    """The last output row and column sit in the last chunk of the position grid (and in the first one's columns next to the
    grid's unused ones): a dz fragment of the wrong chunk, or an x fragment a step early or late, meets zeros."""
    case = _last_row_col(kind)
    (gw, gb), (rw, rb) = case.first, case.ref
    _close(gw, rw)
    _close(gb, rb)
    again = case.fresh()
    assert torch.equal(gw, again[0]) and torch.equal(gb, again[1])
