"""The persistent convolution kernels at shapes where workgroups compute several tiles.

Every convolution on the DRN's hot path starts about as many workgroups as fit on the GPU at once and loops each of them over
output tiles blockIdx.x, + gridDim.x, ...; the kernels carry state from one tile into the next (the next tile's first K step
staged under the current one's last, LDS buffer parities, per-problem scales of z-batched GEMMs, the patch of the next tile,
the tracked maximum).  The single-layer tests of test_gpu_conv.py give no workgroup a second tile; here every form is run at
three tile counts from its launcher's own plan (tests/conv_plan.py, printed per case):

    wrap     one tile more than the grid takes in a round (the least margin)
    full2    exactly two rounds: nothing is staged after the last tile
    ragged   three rounds, the last one short

with B >= 2 (a workgroup's consecutive tiles fall in different images, or problems), short images (tiles of the later rounds
sit on the top and bottom borders, where dilated taps read padding) and a partial last x-tile in every row.  Each case checks:

    accuracy   against float64 of the same operands, at the tolerance of the form's test in test_gpu_conv.py (the light bf16
               kernel: elementwise, one bf16 rounding plus a float32 accumulation term)
    coverage   the output is a NaN-filled caller buffer followed by a NaN guard of at least one tile: afterwards no NaN in the
               output, the guard's bits unchanged; the tracked maximum equals max |y| bit for bit
    position   the last image of the batch is bit-identical to the same image run alone (every output is a fixed-order sum:
               which workgroup computes a tile, or what it computed before, must not change a bit)
"""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
F = torch.nn.functional
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan as cp  # noqa: E402

GUARD = 1 << 16          # elements after every output: one 256 x 256 tile
NAN32, NAN16 = 0x7fc00000, 0x7fc0


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Poisoned(object):
    """a NaN-filled channels-last output (B, C, H, W) and a NaN guard after it"""

    def __init__(self, shape, dtype=torch.float32):
        B, C, H, W = shape
        self.n = B * C * H * W
        self.buf = torch.full((self.n + GUARD,), float('nan'), dtype=dtype, device='cuda')
        self.y = self.buf[:self.n].view(B, H, W, C).permute(0, 3, 1, 2)
        self.bits = (torch.int32, NAN32) if dtype == torch.float32 else (torch.int16, NAN16 - (1 << 16) if NAN16 >= 1 << 15 else NAN16)

    def check(self, what='y'):
        assert not torch.isnan(self.y).any(), '%s: %d outputs never stored, first at (b, c, y, x) %s' % (
            what, int(torch.isnan(self.y).sum()), tuple(torch.nonzero(torch.isnan(self.y))[0].tolist()))
        dt, pat = self.bits
        g = self.buf[self.n:].view(dt)
        assert bool((g == pat).all()), '%s: %d guard elements written' % (what, int((g != pat).sum()))


def _scratch(shape):
    """Winograd scratch with a NaN guard: (tensor, check)"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float('nan'), dtype=torch.float32, device='cuda')

    def check():
        assert bool((buf[n:].view(torch.int32) == NAN32).all()), 'GEMM wrote past its scratch'
    return buf[:n].view(shape), check


def _operands(B, Cin, Cout, H, W, k, res, seed, Ho=None, Wo=None):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.relu(torch.randn((B, Cin, H, W), device='cuda', generator=g)).contiguous(memory_format=torch.channels_last)
    w = torch.randn((Cout, Cin, k, k), device='cuda', generator=g) * (2.0 / (k * k * Cin)) ** 0.5
    bias = torch.randn((Cout,), device='cuda', generator=g)
    r = torch.randn((B, Cout, Ho or H, Wo or W), device='cuda', generator=g).contiguous(memory_format=torch.channels_last) if res else None
    return x, w, bias, r


def _ref64(x, w, bias, r, relu, dil, stride=1):
    pad = dil * (w.shape[2] // 2)
    y = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), stride, pad, dil)
    if r is not None:
        y = y + r.double()
    return torch.relu(y) if relu else y


def _close(y, ref, tol, what='y'):
    scale = float(ref.abs().max())
    err = (y.double() - ref).abs()
    e = float(err.max())
    if e > tol * scale:
        bad = torch.nonzero(err > tol * scale)
        pytest.fail('%s: error %.3e of scale (allowed %.1e) at %d outputs, first (b, c, y, x) %s' % (
            what, e / scale, tol, bad.shape[0], tuple(bad[0].tolist())))


def _amax_equal(am, y):
    assert int(am.view(torch.int32)) == int(y.abs().max().view(torch.int32)), 'tracked maximum %r, max|y| %r' % (
        float(am.view(torch.float32)), float(y.abs().max()))


def _alone(y_all, y_one, b):
    diff = y_all[b:b + 1] != y_one
    assert not bool(diff.any()), 'image %d of the batch differs from the same image alone at %d outputs, first (c, y, x) %s' % (
        b, int(diff.sum()), tuple(torch.nonzero(diff[0])[0].tolist()))


def _show(B, H, W, p):
    print('\n  plan ' + cp.describe(B, H, W, p))


def _sl(t, b):
    return None if t is None else t[b:b + 1]


# ---- the direct kernel (k_conv3x3_f32) and its planes-in-LDS successor (k_conv3x3_p16) ------------------------------------------
@pytest.mark.parametrize('target', cp.TARGETS)
@pytest.mark.parametrize('name', list(cp.DIRECT))
def test_direct_convolution_over_several_rounds(eng, name, target):
    Cin, Cout, taps, dil, res, relu, path, _ = cp.DIRECT[name]
    B, H, W, p = cp.plan_direct(name, target, _n_cu())
    _show(B, H, W, p)
    if name.startswith('p16'):
        assert p['kernel'].startswith('k_conv3x3_p16')
    k = 3 if taps == 9 else 1
    x, w, bias, r = _operands(B, Cin, Cout, H, W, k, res, 31)
    wt = w.permute(0, 2, 3, 1).reshape(Cout, taps, Cin).contiguous()
    ref = _ref64(x, w, bias, r, relu, dil)
    out = Poisoned((B, Cout, H, W))
    if path == 'f32':
        y = eng.conv3x3_f32(x, wt, bias, r, relu, dil, out=out.y)
        y1 = eng.conv3x3_f32(x[B - 1:], wt, bias, _sl(r, B - 1), relu, dil)
        am = None
    else:
        wt2, inv_t = eng.split_planes(wt)
        a_in = eng.amax(x)
        try:
            if path == 'pred':
                eng.debug_set(1, 0)
            y, am = eng.conv3x3_f16s(x, wt2, inv_t, bias, r, relu, dil, amax_in=a_in, out=out.y)
            y1, _ = eng.conv3x3_f16s(x[B - 1:], wt2, inv_t, bias, _sl(r, B - 1), relu, dil, amax_in=a_in)
        finally:
            eng.debug_set(1, 1)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.y.data_ptr()
    out.check()
    _close(y, ref, 4e-6)
    if am is not None:
        _amax_equal(am, y)
    _alone(y, y1, B - 1)
    assert eng.status() == 0


# ---- the stride-2 openers (k_conv3x3_f32<..., S = 2>) ----------------------------------------------------------------------------
@pytest.mark.parametrize('target', cp.TARGETS)
@pytest.mark.parametrize('name', list(cp.STRIDE2))
def test_stride2_opener_over_several_rounds(eng, name, target):
    Cin, Cout, csplit, split = cp.STRIDE2[name]
    B, Hi, Wi, p = cp.plan_stride2(name, target, _n_cu())
    _show(B, Hi, Wi, p)
    Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
    g = torch.Generator(device='cuda').manual_seed(37)
    x = (torch.relu(torch.randn((B, Cin, Hi, Wi), device='cuda', generator=g)) * 2.3).contiguous(memory_format=torch.channels_last)
    w = torch.randn((csplit, Cin, 3, 3), device='cuda', generator=g) * (2.0 / (9 * Cin)) ** 0.5
    wp = torch.randn((Cout - csplit, Cin, 1, 1), device='cuda', generator=g) * (2.0 / Cin) ** 0.5
    b = torch.randn((Cout,), device='cuda', generator=g)
    wc = torch.zeros((Cout, 9, Cin), device='cuda')
    wc[:csplit] = w.permute(0, 2, 3, 1).reshape(csplit, 9, Cin)
    wc[csplit:, 4] = wp.reshape(Cout - csplit, Cin)
    o1 = Poisoned((B, csplit, Ho, Wo))
    o2 = Poisoned((B, Cout - csplit, Ho, Wo)) if csplit < Cout else None
    if split:
        wt2, inv_t = eng.split_planes(wc)
        a_in = eng.amax(x)
        y, y2, am = eng.conv3x3_s2_f16s(x, wt2, inv_t, b, csplit, True, amax_in=a_in, out=o1.y, out2=o2 and o2.y)
        z, z2, _ = eng.conv3x3_s2_f16s(x[B - 1:], wt2, inv_t, b, csplit, True, amax_in=a_in)
        tol = 4e-6
    else:
        y, y2 = eng.conv3x3_s2_f32(x, wc, b, csplit, True, out=o1.y, out2=o2 and o2.y)
        z, z2 = eng.conv3x3_s2_f32(x[B - 1:], wc, b, csplit, True)
        am, tol = None, 3e-6
    torch.cuda.synchronize()
    o1.check()
    _close(y, torch.relu(F.conv2d(x.double(), w.double(), b[:csplit].double(), 2, 1)), tol)
    _alone(y, z, B - 1)
    if am is not None:
        _amax_equal(am, y)
    if o2 is not None:
        o2.check('y2')
        _close(y2, F.conv2d(x.double(), wp.double(), b[csplit:].double(), 2, 0), tol, 'y2')
        _alone(y2, z2, B - 1)
    assert eng.status() == 0


# ---- the Winograd GEMMs: k_gemm_f16x3_stag<256,256> / k_gemm_f16x3<128,128> (F(4x4) split planes) and the float32 form ------------
@pytest.mark.parametrize('target', cp.TARGETS)
@pytest.mark.parametrize('name', list(cp.WINO))
def test_winograd_gemms_over_several_rounds(eng, name, target):
    Cin, Cout, dil, res, relu, tile, split = cp.WINO[name]
    B, H, W, p = cp.plan_wino(name, target, _n_cu(), eng._lib)
    _show(B, H, W, p)
    npos = (tile + 2) ** 2
    T = p['rows']
    x, w, bias, r = _operands(B, Cin, Cout, H, W, 3, res, 41)
    ref = _ref64(x, w, bias, r, relu, dil)
    out = Poisoned((B, Cout, H, W))
    v, vcheck = _scratch((npos, T, Cin))
    m, mcheck = _scratch((npos, T, Cout))
    v.zero_()
    if split:
        u2, cs = eng.winograd_weights_split(w)
        a_in = eng.amax(x)
        y, am = eng.conv3x3_wino_f16s(x, u2, cs, bias, r, relu, dil, amax_in=a_in, out=out.y, scratch=(v, m))
        y1, _ = eng.conv3x3_wino_f16s(x[B - 1:], u2, cs, bias, _sl(r, B - 1), relu, dil, amax_in=a_in)
        tol = 1e-5
    else:
        u = eng.winograd_weights(w, tile)
        y = eng.conv3x3_wino_f32(x, u, bias, r, relu, dil, out=out.y, scratch=(v, m))
        y1 = eng.conv3x3_wino_f32(x[B - 1:], u, bias, _sl(r, B - 1), relu, dil)
        am, tol = None, (4e-6 if tile == 2 else 1e-5)
    torch.cuda.synchronize()
    out.check()            # a GEMM tile left out leaves NaN rows in m, which the output transform carries into y
    vcheck()
    mcheck()
    _close(y, ref, tol)
    if am is not None:
        _amax_equal(am, y)
    _alone(y, y1, B - 1)
    assert eng.status() == 0


# ---- the thin DRN-C convolutions (k_conv_small_f16x3) and layer 2 of DRN-D (k_drn_layer2_f16x3) ----------------------------------
@pytest.mark.parametrize('target', cp.TARGETS)
@pytest.mark.parametrize('name', list(cp.SMALL))
def test_thin_convolution_over_several_rounds(eng, name, target):
    Cin, Cout, stride, proj, res, relu = cp.SMALL[name]
    B, H, W, p = cp.plan_small(name, target, _n_cu())
    _show(B, H, W, p)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    g = torch.Generator(device='cuda').manual_seed(43)
    x = (torch.relu(torch.randn((B, Cin, H, W), device='cuda', generator=g)) * 1.9).contiguous(memory_format=torch.channels_last)
    w = torch.randn((Cout, Cin, 3, 3), device='cuda', generator=g) * (2.0 / (9 * Cin)) ** 0.5
    wd = torch.randn((32, Cin, 1, 1), device='cuda', generator=g) * (2.0 / Cin) ** 0.5 if proj else None
    bias = torch.randn((Cout + (32 if proj else 0),), device='cuda', generator=g)
    r = torch.randn((B, Cout, Ho, Wo), device='cuda', generator=g).contiguous(memory_format=torch.channels_last) if res else None
    wp, inv_t = eng.small_planes(w, wd)
    a_in = eng.amax(x)
    o1 = Poisoned((B, Cout, Ho, Wo))
    o2 = Poisoned((B, 32, Ho, Wo)) if proj else None
    y, y2 = eng.conv_small_f16s(x, wp, inv_t, bias, Cout, stride, 32 if proj else 0, r, relu, amax_in=a_in, out=o1.y, out2=o2 and o2.y)
    z, z2 = eng.conv_small_f16s(x[B - 1:], wp, inv_t, bias, Cout, stride, 32 if proj else 0, _sl(r, B - 1), relu, amax_in=a_in)
    torch.cuda.synchronize()
    o1.check()
    ref = F.conv2d(x.double(), w.double(), bias[:Cout].double(), stride, 1)
    if res:
        ref = ref + r.double()
    _close(y, torch.relu(ref) if relu else ref, 3e-6)
    _amax_equal(y._spa_amax, y)
    _alone(y, z, B - 1)
    if proj:
        o2.check('y2')
        _close(y2, F.conv2d(x.double(), wd.double(), bias[Cout:].double(), stride, 0), 3e-6, 'y2')
        _alone(y2, z2, B - 1)
    assert eng.status() == 0


@pytest.mark.parametrize('target', cp.TARGETS)
def test_drn_layer2_over_several_rounds(eng, target):
    B, H, W, p = cp.plan_layer2(target, _n_cu())
    _show(B, H, W, p)
    g = torch.Generator(device='cuda').manual_seed(47)
    x = (torch.relu(torch.randn((B, 16, H, W), device='cuda', generator=g)) * 1.7).contiguous(memory_format=torch.channels_last)
    w = torch.randn((32, 16, 3, 3), device='cuda', generator=g) * (2.0 / 144) ** 0.5
    b = torch.randn((32,), device='cuda', generator=g)
    wp, inv_t = eng.layer2_planes(w)
    a_in = eng.amax(x)
    out = Poisoned((B, 32, (H + 1) // 2, (W + 1) // 2))
    y = eng.drn_layer2_f16s(x, wp, inv_t, b, amax_in=a_in, out=out.y)
    z = eng.drn_layer2_f16s(x[B - 1:], wp, inv_t, b, amax_in=a_in)
    torch.cuda.synchronize()
    out.check()
    _close(y, torch.relu(F.conv2d(x.double(), w.double(), b.double(), 2, 1)), 3e-6)
    _amax_equal(y._spa_amax, y)
    _alone(y, z, B - 1)
    assert eng.status() == 0


# ---- the light bf16 kernel (k_conv_bf16_light): persistent strips of 64 pixels, several channel blocks ----------------------------
@pytest.mark.parametrize('target', cp.TARGETS)
@pytest.mark.parametrize('name', list(cp.LIGHT))
def test_light_bf16_convolution_over_several_rounds(eng, name, target):
    Cin, Cout, taps, stride, dil, res, relu = cp.LIGHT[name]
    B, H, W, p = cp.plan_light(name, target, _n_cu())
    _show(B, H, W, p)
    assert p['nblk'] > 1
    k = 3 if taps == 9 else 1
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    g = torch.Generator(device='cuda').manual_seed(53)
    x = torch.randn((B, Cin, H, W), device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn((Cout, Cin, k, k), device='cuda', generator=g) * (2.0 / (taps * Cin)) ** 0.5).to(torch.bfloat16)
    bias = torch.randn((Cout,), device='cuda', generator=g)
    r = torch.randn((B, Cout, Ho, Wo), device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last) if res else None
    wt = w.permute(0, 2, 3, 1).reshape(Cout, taps, Cin).contiguous()
    out = Poisoned((B, Cout, Ho, Wo), torch.bfloat16)
    y = eng.conv_bf16_light(x, wt, bias, r, relu, stride, dil, out=out.y)
    z = eng.conv_bf16_light(x[B - 1:], wt, bias, _sl(r, B - 1), relu, stride, dil)
    torch.cuda.synchronize()
    out.check()
    pad = dil if taps == 9 else 0
    K = taps * Cin + 2
    gamma = K * 2.0 ** -24 / (1 - K * 2.0 ** -24)
    for b in range(B):              # one image at a time: the float64 operands of the largest shapes would not fit in 1 GB
        xb, wd = x[b:b + 1].double(), w.double()
        ref = F.conv2d(xb, wd, bias.double(), stride, pad, dil)
        mag = F.conv2d(xb.abs(), wd.abs(), bias.double().abs(), stride, pad, dil)        # sum |x w| + |bias|
        if res:
            ref = ref + r[b:b + 1].double()
            mag = mag + r[b:b + 1].double().abs()
        if relu:
            ref = torch.relu(ref)
        # float32 accumulation of K products, the bias and the residual in any order: gamma_(K+2) sum |terms|; then one
        # rounding to bf16 (8 significant bits: unit roundoff 2^-8) of the float32 value
        acc = gamma * mag
        bound = 2.0 ** -8 * (ref.abs() + acc) + acc
        yb = y[b:b + 1].double()
        excess = (yb - ref).abs() - bound
        if bool((excess > 0).any()):
            i = tuple(torch.nonzero(excess > 0)[0].tolist())
            pytest.fail('image %d: %d outputs outside the elementwise bound, first (b, c, y, x) %s: %r vs %r (bound %.3e)' % (
                b, int((excess > 0).sum()), i, float(yb[i]), float(ref[i]), float(bound[i])))
    _alone(y, z, B - 1)
    eng.raise_on_status()
