"""GPU tests of the direct MFMA convolutions of the DRN on operands whose result is known bit for bit (tests/conv_exact.py has the
argument, the regimes and the premise): small integers, power-of-two scales, every partial sum inside 24 bits of one unit, so the
kernel's float32 accumulation is exact in any order and the output is the float64 reference rounded once.  Every comparison is
torch.equal over the whole output — a dropped, doubled or misplaced term, a wrong border pixel, a stale LDS buffer or a rounding
other than to nearest even changes at least one integer.  The cases (conv_exact.BF16, LIGHT, F16S_*, S2, WIDE_*) are the smallest
shapes that reach the branch named beside them; test_conv_exact_cpu.py checks each case's bound without a GPU.

Covered: spa_conv3x3_bf16 (k_conv3x3_bf16 at the 64 and 128 tiles, k_conv3x3_bf16_stag), spa_conv_bf16_light (every instantiation),
spa_conv3x3_f16s / spa_conv1x1_f16s (k_conv3x3_p16, k_conv3x3_f32<SPLIT>), spa_conv3x3_s2_f16s (k_conv3x3_s2_tile and the generic
kernel), and one 'wide' case each of spa_conv3x3_f32 / spa_conv1x1_f32, spa_conv3x3_s2_f32, spa_conv_small_f16s, spa_drn_layer2_f32
and spa_drn_layer2_f16s.  The Winograd paths have tests/test_gpu_wino_exact.py; left out because their arithmetic is not exact
on integers: the fused stems (mean / std normalisation)."""
import importlib
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact as ce  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


def _cl(t, dtype):
    """a (B,C,H,W) operand on the GPU in channels-last storage"""
    return None if t is None else t.to(dtype).cuda().contiguous(memory_format=torch.channels_last)


def _dev(t, dtype=torch.float32):
    return t.to(dtype).cuda().contiguous()


def _ids(k):
    return '-'.join(str(int(v)) if isinstance(v, bool) else str(v) for v in k)


def _amax_is_the_outputs(am, y):
    assert int(am.view(torch.int32)) == int(y.abs().max().reshape(1).view(torch.int32)), 'tracked maximum'


# ---- spa_conv3x3_bf16 -----------------------------------------------------------------------------------------------------------
def _run_bf16(eng, c):
    bf = torch.bfloat16
    return eng.conv3x3_bf16(_cl(c.x, bf), _dev(c.wt(), bf), _dev(c.bias), _cl(c.res, bf), c.relu, c.dil)


@pytest.mark.parametrize('regime', ['unit', 'wide'])
@pytest.mark.parametrize('shape', ce.BF16, ids=_ids)
def test_conv3x3_bf16_is_exact(eng, shape, regime):
    B, Cin, Cout, H, W, dil, res, relu = shape
    c = ce.case(regime, B, Cin, Cout, H, W, 9, 1, dil, res, relu)
    y = _run_bf16(eng, c)
    assert y.is_contiguous(memory_format=torch.channels_last)
    ce.check(y, c.ref(torch.bfloat16)[0], 'spa_conv3x3_bf16 %s %s' % (regime, shape))
    assert eng.status() == 0


@pytest.mark.parametrize('regime', ['unit', 'wide'])
def test_conv3x3_bf16_staggered_kernel_gives_the_same_exact_bits_every_time(eng, regime):
    """k_conv3x3_bf16_stag counts its waits by hand and runs the two waves of a SIMD half a period apart: a race would show as a
    run that differs.  Six runs of the 512 -> 512 layer (72 K steps), each the exact result."""
    B, Cin, Cout, H, W, dil, res, relu = ce.BF16_REPEATED
    c = ce.case(regime, B, Cin, Cout, H, W, 9, 1, dil, res, relu)
    ref = c.ref(torch.bfloat16)[0].cuda()
    bf = torch.bfloat16
    x, wt, bias = _cl(c.x, bf), _dev(c.wt(), bf), _dev(c.bias)
    for rep in range(6):
        ce.check(eng.conv3x3_bf16(x, wt, bias, None, relu, dil), ref, 'repetition %d' % rep)
    assert eng.status() == 0


def test_the_check_sees_one_term_through_the_kernels(eng):
    """the comparison is as sharp on the GPU as test_conv_exact_cpu.py shows it on the CPU: the 512 -> 512 bf16 layer run on weights
    with ONE (channel, tap) term zeroed, and the 128 -> 128 split-plane layer run with the weights' low plane zeroed, are rejected"""
    B, Cin, Cout, H, W, dil, res, relu = ce.BF16_REPEATED
    c = ce.case('unit', B, Cin, Cout, H, W, 9, 1, dil, res, relu)
    bf = torch.bfloat16
    wt = _dev(c.wt(), bf)
    wt[:, 2, 137] = 0                                      # tap (ky 0, kx 2) of input channel 137, every output channel
    with pytest.raises(AssertionError, match='outputs differ'):
        ce.check(eng.conv3x3_bf16(_cl(c.x, bf), wt, _dev(c.bias), None, relu, dil), c.ref(bf)[0])
    B, C, H, W, dil, res, relu = ce.F16S_3X3[4]
    c = ce.case('planes_w', B, C, C, H, W, 9, 1, dil, res, relu)
    wt2, inv_t = eng.split_planes(_dev(c.wt()))
    wt2[:, :, :, 1] = 0
    y, _ = eng.conv3x3_f16s(_cl(c.x, torch.float32), wt2, inv_t, _dev(c.bias), _cl(c.res, torch.float32), relu, dil)
    with pytest.raises(AssertionError, match='outputs differ'):
        ce.check(y, c.ref(torch.float32)[0])
    assert eng.status() == 0


# ---- spa_conv_bf16_light --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ['unit', 'wide'])
@pytest.mark.parametrize('shape', ce.LIGHT, ids=_ids)
def test_conv_bf16_light_is_exact(eng, shape, regime):
    Cin, Cout, taps, stride, dil, res, relu, B, H, W = shape
    c = ce.case(regime, B, Cin, Cout, H, W, taps, stride, dil, res, relu)
    bf = torch.bfloat16
    y = eng.conv_bf16_light(_cl(c.x, bf), _dev(c.wt(), bf), _dev(c.bias), _cl(c.res, bf), relu, stride, dil)
    ce.check(y, c.ref(bf)[0], 'spa_conv_bf16_light %s %s' % (regime, shape))
    eng.raise_on_status()


# ---- spa_conv3x3_f16s / spa_conv1x1_f16s ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ['planes_x', 'planes_w'])
@pytest.mark.parametrize('shape', ce.F16S_3X3, ids=_ids)
def test_conv3x3_split_planes_is_exact_in_both_kernels(eng, shape, regime):
    """k_conv3x3_p16 (spa_debug_set(ctx, 1, 1), the default) and the kernel it replaced, k_conv3x3_f32<SPLIT> (1, 0): the exact
    result from both, and the tracked maximum is the output's"""
    B, C, H, W, dil, res, relu = shape
    c = ce.case(regime, B, C, C, H, W, 9, 1, dil, res, relu)
    x, bias, r = _cl(c.x, torch.float32), _dev(c.bias), _cl(c.res, torch.float32)
    wt2, inv_t = eng.split_planes(_dev(c.wt()))
    assert bool((wt2[:, :, :, 1] != 0).any()) == (regime == 'planes_w')           # who carries the low plane
    ref = c.ref(torch.float32)[0].cuda()
    try:
        for on, kernel in ((1, 'k_conv3x3_p16'), (0, 'k_conv3x3_f32<SPLIT>')):
            eng.debug_set(1, on)
            y, am = eng.conv3x3_f16s(x, wt2, inv_t, bias, r, relu, dil)
            ce.check(y, ref, '%s %s %s' % (kernel, regime, shape))
            _amax_is_the_outputs(am, y)
    finally:
        eng.debug_set(1, 1)
    assert eng.status() == 0


@pytest.mark.parametrize('regime', ['planes_x', 'planes_w'])
@pytest.mark.parametrize('shape', ce.F16S_1X1, ids=_ids)
def test_conv1x1_split_planes_is_exact(eng, shape, regime):
    B, Cin, Cout, H, W, res, relu = shape
    c = ce.case(regime, B, Cin, Cout, H, W, 1, 1, 1, res, relu)
    wt2, inv_t = eng.split_planes(_dev(c.wt()))
    y, am = eng.conv3x3_f16s(_cl(c.x, torch.float32), wt2, inv_t, _dev(c.bias), _cl(c.res, torch.float32), relu, 1)
    ce.check(y, c.ref(torch.float32)[0], 'spa_conv1x1_f16s %s %s' % (regime, shape))
    _amax_is_the_outputs(am, y)
    assert eng.status() == 0


# ---- spa_conv3x3_s2_f16s --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ['planes_x', 'planes_w'])
@pytest.mark.parametrize('shape', ce.S2, ids=_ids)
def test_conv3x3_stride2_with_projection_is_exact_in_both_kernels(eng, shape, regime):
    """the stride-2 opener and the block's 1x1 stride-2 projection in one pass: k_conv3x3_s2_tile (spa_debug_set(ctx, 3, 1), the
    default) and the generic kernel (3, 0); y and y2 are both the exact result"""
    B, Cin, Cout, Hi, Wi = shape
    c = ce.case(regime, B, Cin, Cout, Hi, Wi, 9, 2, 1, False, True, Cout)
    x, bias = _cl(c.x, torch.float32), _dev(c.bias_all())
    wt2, inv_t = eng.split_planes(_dev(c.wt_proj()))
    ref, ref2 = (t.cuda() for t in c.ref(torch.float32))
    try:
        for on, kernel in ((1, 'k_conv3x3_s2_tile'), (0, 'k_conv3x3_f32<SPLIT, S = 2>')):
            eng.debug_set(3, on)
            y, y2, am = eng.conv3x3_s2_f16s(x, wt2, inv_t, bias, Cout, True)
            ce.check(y, ref, '%s y %s %s' % (kernel, regime, shape))
            ce.check(y2, ref2, '%s y2 %s %s' % (kernel, regime, shape))
            _amax_is_the_outputs(am, y)
    finally:
        eng.debug_set(3, 1)
    assert eng.status() == 0


# ---- one 'wide' case each of the other direct forms -----------------------------------------------------------------------------
def test_conv3x3_f32_is_exact(eng):
    B, Cin, Cout, H, W, dil, res, relu = ce.WIDE_F32_3X3
    c = ce.case('wide', B, Cin, Cout, H, W, 9, 1, dil, res, relu)
    y = eng.conv3x3_f32(_cl(c.x, torch.float32), _dev(c.wt()), _dev(c.bias), _cl(c.res, torch.float32), relu, dil)
    ce.check(y, c.ref(torch.float32)[0], 'spa_conv3x3_f32')
    B, Cin, Cout, H, W = ce.WIDE_F32_1X1
    c = ce.case('wide', B, Cin, Cout, H, W, 1, 1, 1, False, False)
    y = eng.conv3x3_f32(_cl(c.x, torch.float32), _dev(c.wt()), _dev(c.bias), None, False, 1)
    ce.check(y, c.ref(torch.float32)[0], 'spa_conv1x1_f32')
    assert eng.status() == 0


def test_conv3x3_stride2_float32_instructions_is_exact(eng):
    B, Cin, Cout, Hi, Wi = ce.WIDE_S2_F32
    c = ce.case('wide', B, Cin, Cout, Hi, Wi, 9, 2, 1, False, True, Cout)
    y, y2 = eng.conv3x3_s2_f32(_cl(c.x, torch.float32), _dev(c.wt_proj()), _dev(c.bias_all()), Cout, True)
    ref, ref2 = c.ref(torch.float32)
    ce.check(y, ref, 'spa_conv3x3_s2_f32 y')
    ce.check(y2, ref2, 'spa_conv3x3_s2_f32 y2')
    assert eng.status() == 0


@pytest.mark.parametrize('shape', ce.WIDE_SMALL, ids=_ids)
def test_thin_convolution_is_exact(eng, shape):
    Cin, Cout, stride, proj, res, relu, B, H, W = shape
    c = ce.case('wide', B, Cin, Cout, H, W, 9, stride, 1, res, relu, proj)
    wp, inv_t = eng.small_planes(c.w.float().cuda(), c.wd.float().cuda() if proj else None)
    y, y2 = eng.conv_small_f16s(_cl(c.x, torch.float32), wp, inv_t, _dev(c.bias_all()), Cout, stride, proj, _cl(c.res, torch.float32), relu)
    ref, ref2 = c.ref(torch.float32)
    ce.check(y, ref, 'spa_conv_small_f16s y')
    _amax_is_the_outputs(y._spa_amax, y)
    if proj:
        ce.check(y2, ref2, 'spa_conv_small_f16s y2')
    assert eng.status() == 0


def test_drn_layer2_is_exact_in_both_forms(eng):
    B, H, W = ce.WIDE_LAYER2
    c = ce.case('wide', B, 16, 32, H, W, 9, 2, 1, False, True)
    ref = c.ref(torch.float32)[0].cuda()
    x, bias = _cl(c.x, torch.float32), _dev(c.bias)
    y = eng.drn_layer2_f32(x, _dev(c.w.permute(2, 3, 1, 0).reshape(9, 16, 32)), bias)
    ce.check(y, ref, 'spa_drn_layer2_f32')
    wp, inv_t = eng.layer2_planes(c.w.float().cuda())
    y = eng.drn_layer2_f16s(x, wp, inv_t, bias)
    ce.check(y, ref, 'spa_drn_layer2_f16s')
    _amax_is_the_outputs(y._spa_amax, y)
    assert eng.status() == 0
