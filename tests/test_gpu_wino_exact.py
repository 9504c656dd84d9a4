"""GPU tests of the Winograd convolutions on operands whose result is known bit for bit (tests/wino_exact.py has the argument, the
premises, the regimes and their bounds): integer pixels, weights 225 k (F(4x4,3x3)) or k (F(2x2,3x3)), every scale a power of
two, every partial sum inside 24 bits of its addends' smallest unit, so the float32 arithmetic of the transforms and of the
matrix instructions is exact in any order and the output IS the float64 reference.  Every comparison is torch.equal over the whole
output, and for the split form over the tracked maximum too: one dropped, doubled or misplaced (channel, position) term, a wrong
low plane, scale, tile decode, halo or clipped row changes at least one output.  test_wino_exact_cpu.py shows that without a GPU.

Covered: spa_conv3x3_wino4_f16s under spa_debug_set key 4 = 0, 1 and 2 (k_wino4_in with float32 V and with planes, k_gemm_f16x3,
k_gemm_f16x3_stag with and without planes, k_wino4_out_s), spa_conv3x3_wino4_f32 and spa_conv3x3_wino_f32 (k_wino4_in / k_wino_in,
the float32 GEMM, k_wino4_out / k_wino_out).  Every call runs twice into a NaN-poisoned output with a NaN guard behind it and
fresh NaN-filled scratch: rows T .. Tpad of V are never written, and nothing may read their products."""
import importlib
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_ref as sr  # noqa: E402
import wino_exact as we  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.debug_set(4, 2)
    e.close()


def _cl(t):
    """a (B,C,H,W) operand on the GPU, float32 in channels-last storage"""
    return None if t is None else t.float().cuda().contiguous(memory_format=torch.channels_last)


def _out(c):
    """(channels-last NaN view (B,Cout,H,W), its buffer with the guard, the view's length)"""
    B, Cin, Cout, H, W = c.shape
    view, buf = sr.poisoned((B, H, W, Cout))
    return view.permute(0, 3, 1, 2), buf, view.numel()


def _scratch(c):
    """V and M of one call, NaN everywhere: what the kernels do not write stays NaN"""
    n2, Tpad = (c.tile + 2) ** 2, c.geom.Tpad
    return (torch.full((n2, Tpad, c.shape[1]), float('nan'), device='cuda'), torch.full((n2, Tpad, c.shape[2]), float('nan'), device='cuda'))


def _word(c):
    return torch.tensor([c.amax_word], dtype=torch.int32, device='cuda')


def _split_form(eng, c, ref, what, u2=None, keys=(0, 1, 2)):
    """spa_conv3x3_wino4_f16s under every operand path, twice each: y and the amax word are the reference's, the guard is whole"""
    x, bias, r = _cl(c.x), c.bias.float().cuda(), _cl(c.res)
    u2 = c.u2.cuda() if u2 is None else u2
    want = int(ref.abs().max().reshape(1).view(torch.int32))
    if not c.amax2:
        assert int(eng.amax(x)) == c.amax_word, 'k_amax'
    try:
        for key in keys:
            eng.debug_set(4, key)
            for rep in range(2):
                out, buf, n = _out(c)
                y, am = eng.conv3x3_wino_f16s(x, u2, c.cs, bias, r, c.relu, c.dil, amax_in=_word(c), out=out, scratch=_scratch(c))
                we.check(y, ref, '%s, key 4 = %d, call %d' % (what, key, rep))
                assert int(am) == want, 'tracked maximum (key 4 = %d)' % key
                sr.check_guard(buf, n)
    finally:
        eng.debug_set(4, 2)
    assert eng.status() == 0


def _float_form(eng, c, ref, what, u=None):
    """spa_conv3x3_wino4_f32 / spa_conv3x3_wino_f32, twice"""
    x, bias, r = _cl(c.x), c.bias.float().cuda(), _cl(c.res)
    u = c.u.cuda() if u is None else u
    for rep in range(2):
        out, buf, n = _out(c)
        y = eng.conv3x3_wino_f32(x, u, bias, r, c.relu, c.dil, out=out, scratch=_scratch(c))
        we.check(y, ref, '%s, call %d' % (what, rep))
        sr.check_guard(buf, n)
    assert eng.status() == 0


@pytest.mark.parametrize('key', we.F4, ids=we.ident)
def test_wino4_split_planes_is_exact_under_every_operand_path(eng, key):
    c = we.f4(key)
    _split_form(eng, c, c.ref().cuda(), 'spa_conv3x3_wino4_f16s %s' % we.ident(key))


@pytest.mark.parametrize('key', [k for k in we.F4 if not k[7]], ids=we.ident)
def test_wino4_float32_is_exact(eng, key):
    c = we.f4(key)
    _float_form(eng, c, c.ref().cuda(), 'spa_conv3x3_wino4_f32 %s' % we.ident(key))


@pytest.mark.parametrize('key', we.F2, ids=we.ident)
def test_wino2_float32_is_exact(eng, key):
    c = we.f2(key)
    _float_form(eng, c, c.ref().cuda(), 'spa_conv3x3_wino_f32 %s' % we.ident(key))


def test_per_tap_reference_on_the_device_is_the_cpu_convolution():
    """the reference of the planned shape below (9 per-tap float64 matrix products on the device), held to F.conv2d on the CPU"""
    for key in (we.F4[2], we.F4[13]):
        c = we.f4(key)
        assert torch.equal(c.ref('cuda', taps=True).cpu(), c.ref())


def test_every_gemm_workgroup_computes_several_tiles(eng):
    """the smallest shape conv_plan finds at which every workgroup of k_gemm_f16x3_stag<256,256> ends at its second tile"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    c, p = we.large_case(n_cu, eng._lib)
    print('B %d  H %d  W %d  tiles %d  workgroups %d' % (c.shape[0], c.shape[3], c.shape[4], p['tiles'], p['slots']))
    assert p['slots'] < p['tiles'] <= 2 * p['slots']
    ref = c.ref('cuda', taps=True)
    _split_form(eng, c, ref, 'spa_conv3x3_wino4_f16s planned %s' % (c.shape,))
    _float_form(eng, c, ref, 'spa_conv3x3_wino4_f32 planned %s' % (c.shape,))


def test_the_check_sees_a_low_plane_and_one_element_of_u_through_the_kernels(eng):
    """the comparison is as sharp on the GPU as test_wino_exact_cpu.py shows it on the CPU: the 'planes_w' layer run on u2 with its
    low plane zeroed, and the 512 -> 512 layer run on U with ONE element of 36 x 512 x 512 zeroed, are rejected"""
    c = we.f4(we.MUTANT_LOW)
    u2 = c.u2.cuda()
    u2[:, :, :, 1, :] = 0
    with pytest.raises(AssertionError, match='outputs differ'):
        _split_form(eng, c, c.ref().cuda(), 'low plane zeroed', u2=u2, keys=(2,))
    c = we.f4(we.MUTANT_TERM)
    assert c.shape[1] == 512
    z = 22
    co, ci = (int(v) for v in (c.u[z] != 0).nonzero()[54321])             # some non-zero element of that position
    for keys in ((0,), (2,)):
        u2 = c.u2.cuda()
        u2[z, co, ci // 32, :, ci % 32] = 0
        with pytest.raises(AssertionError, match='outputs differ'):
            _split_form(eng, c, c.ref().cuda(), 'one element of U zeroed', u2=u2, keys=keys)
    u = c.u.cuda()
    u[z, co, ci] = 0
    with pytest.raises(AssertionError, match='outputs differ'):
        _float_form(eng, c, c.ref().cuda(), 'one element of U zeroed', u=u)
    assert eng.status() == 0
