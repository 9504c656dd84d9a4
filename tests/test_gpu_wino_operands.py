"""The operand path of the split-plane Winograd layers (Engine.conv3x3_wino_f16s) behind spa_debug_set key 4:
0 = tiles numbered sub-grid by sub-grid and float32 V (the forms before round 8), 1 = the sub-grids of a pixel row interleaved in
the numbering (dilation > 2), 2 = that numbering and V written by k_wino4_in as the GEMM's half-precision planes (Cout from 512 on).  The row order of V and M means nothing to the
GEMM, and the planes are made by the GEMM's own split function from the same values, so all three give the SAME BITS, in
y and in the tracked maximum; and each is the float64 convolution at the tolerance tests/test_gpu_conv.py has for this entry
point (1e-5 of the map's scale).  (Dilation 2 keeps the old numbering under every key — profiles/r8_wino_operands_ab.txt — so
on the GPU the interleaved decode runs in the dilation-4 cases; tests/test_wino_numbering_cpu.py checks it for 1, 2 and 4.)"""
import importlib

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
F = torch.nn.functional


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.debug_set(4, 2)
    e.close()


def _operands(B, Cin, Cout, H, W, res, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = (torch.relu(torch.randn((B, Cin, H, W), device='cuda', generator=g)) * 3.7).contiguous(memory_format=torch.channels_last)
    w = torch.randn((Cout, Cin, 3, 3), device='cuda', generator=g) * (2.0 / (9 * Cin)) ** 0.5
    bias = torch.randn((Cout,), device='cuda', generator=g)
    r = torch.randn((B, Cout, H, W), device='cuda', generator=g).contiguous(memory_format=torch.channels_last) if res else None
    return x, w, bias, r


def _ref64(x, w, bias, r, relu, dil):
    y = F.conv2d(x.double(), w.double(), bias.double(), 1, dil, dil)
    if r is not None:
        y = y + r.double()
    return torch.relu(y) if relu else y


def _three_forms(eng, x, w, bias, r, relu, dil):
    """y and the amax word for key 4 = 0, 1, 2: equal bits, and the float64 convolution at 1e-5 of its scale"""
    u2, cs = eng.winograd_weights_split(w)
    am = eng.amax(x)
    out = []
    for key in (0, 1, 2):
        eng.debug_set(4, key)
        y, am_out = eng.conv3x3_wino_f16s(x, u2, cs, bias, r, relu, dil, amax_in=am)
        out.append((y.clone(), am_out.clone()))
    eng.debug_set(4, 2)
    (y0, a0), (y1, a1), (y2, a2) = out
    assert torch.equal(y0, y1) and torch.equal(a0, a1), 'the interleaved numbering changed the result'
    assert torch.equal(y0, y2) and torch.equal(a0, a2), 'V as planes changed the result'
    ref = _ref64(x, w, bias, r, relu, dil)
    scale = float(ref.abs().max())
    for y, a in out:
        if scale > 0:
            assert float((y.double() - ref).abs().max()) <= 1e-5 * scale
        assert float(a.view(torch.float32)) == float(y.abs().max())
    return y2, a2


# ragged sub-grids: at d = 4 a 22 x 38 map is 6 x 10 sub-grids (2 x 3 tiles, last row and column partly outside) and a
# 9 x 7 map is less than one tile per sub-grid; Cout 128 takes the 128 x 128 GEMM tile (float32 V under every key, as has Cout 256)
@pytest.mark.parametrize('H,W', [(22, 38), (9, 7)])
@pytest.mark.parametrize('dil', [1, 2, 4])
def test_ragged_subgrids(eng, H, W, dil):
    _three_forms(eng, *_operands(2, 64, 128, H, W, True, 11), True, dil)


# the same maps with 512 output channels: the layers whose V is written as planes (two channel tiles of 256)
@pytest.mark.parametrize('H,W', [(22, 38), (9, 7)])
@pytest.mark.parametrize('dil', [1, 2, 4])
def test_ragged_subgrids_planes(eng, H, W, dil):
    _three_forms(eng, *_operands(2, 64, 512, H, W, True, 12), True, dil)


def test_two_gemm_row_tiles_with_a_padded_last_one(eng):
    """3 x 36 x 52 at d = 1: 351 tiles, Tpad = 512 — rows 351 .. 511 of V are never written and nothing reads their products"""
    assert int(eng._lib.spa_wino4_tiles(3, 36, 52, 1)) == 512
    _three_forms(eng, *_operands(3, 256, 256, 36, 52, False, 13), True, 1)
    _three_forms(eng, *_operands(3, 64, 512, 36, 52, False, 13), True, 1)          # the same rows as planes


@pytest.mark.parametrize('Cin,Cout,dil,res', [(512, 512, 4, True), (256, 512, 2, False)])
def test_bench_channel_counts(eng, Cin, Cout, dil, res):
    _three_forms(eng, *_operands(1, Cin, Cout, 16, 24, res, 14), True, dil)


def test_planes_hostile_magnitudes(eng):
    """input magnitudes from 2^-20 to 2^10 in one tensor (the scale is the position's exact power of two below the tracked
    maximum) and an all-zero image (amax word 0: the `bits == 0` branch of the exponent)"""
    x, w, bias, r = _operands(2, 64, 512, 22, 38, False, 15)
    g = torch.Generator(device='cuda').manual_seed(16)
    e = torch.randint(-20, 11, x.shape, device='cuda', generator=g).float()
    xs = (torch.sign(torch.randn(x.shape, device='cuda', generator=g)) * (1.0 + torch.rand(x.shape, device='cuda', generator=g))
          * torch.exp2(e) * 0.999).contiguous(memory_format=torch.channels_last)
    xs[0, 0, 0, 0] = 2.0 ** -20
    xs[0, 1, 0, 0] = 2.0 ** 10
    _three_forms(eng, xs, w, bias, None, False, 2)
    z = torch.zeros_like(x)
    assert int(eng.amax(z)) == 0
    y, _ = _three_forms(eng, z, w, bias, None, True, 4)
    assert torch.equal(y, torch.relu(bias).view(1, -1, 1, 1).expand_as(y).contiguous(memory_format=torch.channels_last))
