"""The 2-D tile kernel of the stride-2 openers (k_conv3x3_s2_tile, csrc/spa_convs2.hip) behind spa_conv3x3_s2_f16s.

It replaces the generic kernel (k_conv3x3_f32<..., S = 2>, still selectable with Engine.debug_set(3, 0)) for the shapes the networks
use, and is built to feed every accumulator the same matrix instructions in the same order: the outputs and the tracked maximum
must be the generic kernel's bit for bit — on both network shapes, the two mixed ones, the form without a projection, odd sizes,
maps narrower than a tile, a single pixel, a size that gives every persistent workgroup several tiles, and the benchmark's own
layer-3 size.  Each shape is also held to a float64 convolution on its own (the tolerance of
test_gpu_conv.py::test_conv3x3_stride2_with_projection_matches_float64), and an image must get the same bits alone as inside a batch.
"""
import importlib

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
F = torch.nn.functional

GUARD = 1 << 14
NAN32 = 0x7fc00000

# (Cin, csplit, projection, relu)
FORMS = [(32, 64, True, True), (64, 128, True, True), (64, 64, True, True), (32, 128, True, True),
         (32, 128, False, False), (32, 128, False, True), (64, 128, False, False), (64, 128, False, True)]
SIZES = [(64, 128), (63, 127), (65, 130), (17, 33), (1, 1)]
MANY = (130, 1030)           # B = 2: 17 x 17 x 2 tiles of 4 x 32 (Cin 32), 33 x 17 x 2 of 2 x 32 (Cin 64)
B = 2


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.debug_set(3, 1)
    e.close()


def _tiles(Cin, Hi, Wi, nb):
    """tile count of k_conv3x3_s2_tile: 32 output pixels wide, 4 rows (32 input channels) or 2 rows (64) high"""
    th = 4 if Cin == 32 else 2
    Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
    return ((Wo + 31) // 32) * ((Ho + th - 1) // th) * nb


class Poisoned(object):
    """a NaN-filled channels-last output (B, C, H, W) with a NaN guard after it"""

    def __init__(self, shape):
        nb, C, H, W = shape
        self.n = nb * C * H * W
        self.buf = torch.full((self.n + GUARD,), float('nan'), dtype=torch.float32, device='cuda')
        self.y = self.buf[:self.n].view(nb, H, W, C).permute(0, 3, 1, 2)

    def check(self, what):
        assert not torch.isnan(self.y).any(), '%s: %d outputs never stored' % (what, int(torch.isnan(self.y).sum()))
        assert bool((self.buf[self.n:].view(torch.int32) == NAN32).all()), '%s: guard written' % what


def _operands(eng, Cin, csplit, proj, Hi, Wi, nb=B, seed=71):
    """inputs with negative values, exact zeros (a tenth of them) and the largest magnitude, negative, in the last element"""
    g = torch.Generator(device='cuda').manual_seed(seed + Cin + csplit + Hi * 7 + Wi)
    x = torch.randn((nb, Cin, Hi, Wi), device='cuda', generator=g) * 2.3
    x = x * (torch.rand((nb, Cin, Hi, Wi), device='cuda', generator=g) >= 0.1)
    x[0, 0, 0, 0] = 0.0
    x[nb - 1, Cin - 1, Hi - 1, Wi - 1] = -(x.abs().max() + 0.5)
    x = x.contiguous(memory_format=torch.channels_last)
    Cout = csplit * (2 if proj else 1)
    w = torch.randn((csplit, Cin, 3, 3), device='cuda', generator=g) * (2.0 / (9 * Cin)) ** 0.5
    wd = torch.randn((csplit, Cin, 1, 1), device='cuda', generator=g) * (2.0 / Cin) ** 0.5 if proj else None
    b = torch.randn((Cout,), device='cuda', generator=g)
    wc = torch.zeros((Cout, 9, Cin), device='cuda')
    wc[:csplit] = w.permute(0, 2, 3, 1).reshape(csplit, 9, Cin)
    if proj:
        wc[csplit:, 4] = wd.reshape(csplit, Cin)
    wt2, inv_t = eng.split_planes(wc)
    am = eng.amax(x)
    assert int(am.view(torch.int32)) == int(x.abs().max().view(torch.int32))
    assert bool((x == 0).any()) and bool((x < 0).any())
    return x, w, wd, b, wt2, inv_t, am


def _run(eng, key, x, wt2, inv_t, b, csplit, proj, relu, am):
    nb, _, Hi, Wi = x.shape
    Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
    o1 = Poisoned((nb, csplit, Ho, Wo))
    o2 = Poisoned((nb, csplit, Ho, Wo)) if proj else None
    try:
        eng.debug_set(3, key)
        y, y2, a = eng.conv3x3_s2_f16s(x, wt2, inv_t, b, csplit, relu, amax_in=am, out=o1.y, out2=o2.y if proj else None)
        torch.cuda.synchronize()
    finally:
        eng.debug_set(3, 1)
    o1.check('y (key 3 = %d)' % key)
    if proj:
        o2.check('y2 (key 3 = %d)' % key)
    else:
        assert y2 is None
    assert eng.status() == 0
    return y, y2, a


def _same_bits(a, b, what):
    ai, bi = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    if not torch.equal(ai, bi):
        d = ai != bi
        pytest.fail('%s: %d of %d words differ, first at %s' % (what, int(d.sum()), d.numel(), tuple(torch.nonzero(d)[0].tolist())))


def _cases():
    out = []
    for form in FORMS:
        for size in SIZES + [MANY]:
            out.append(form + size)
    for form in FORMS:
        if form[0] == 32:
            out.append(form + (512, 1024))           # the benchmark's layer-3 input
    return out


@pytest.mark.parametrize('Cin,csplit,proj,relu,Hi,Wi', _cases())
def test_tile_kernel_has_the_bits_of_the_generic_kernel(eng, Cin, csplit, proj, relu, Hi, Wi):
    if (Hi, Wi) == MANY:
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        assert _tiles(Cin, Hi, Wi, B) > 2 * n_cu, 'every workgroup must get several tiles: %d tiles, %d CUs' % (_tiles(Cin, Hi, Wi, B), n_cu)
    x, w, wd, b, wt2, inv_t, am = _operands(eng, Cin, csplit, proj, Hi, Wi)
    y0, y20, a0 = _run(eng, 0, x, wt2, inv_t, b, csplit, proj, relu, am)
    for rep in range(2):                             # (the second run: the same bits again)
        y1, y21, a1 = _run(eng, 1, x, wt2, inv_t, b, csplit, proj, relu, am)
        _same_bits(y0, y1, 'y, run %d' % rep)
        if proj:
            _same_bits(y20, y21, 'y2, run %d' % rep)
        assert int(a0) == int(a1), 'amax_out %r vs %r' % (int(a0), int(a1))
    assert int(a1) == int(y1.abs().max().view(torch.int32))


@pytest.mark.parametrize('Cin,csplit,proj,relu,Hi,Wi', _cases())
def test_tile_kernel_matches_float64(eng, Cin, csplit, proj, relu, Hi, Wi):
    x, w, wd, b, wt2, inv_t, am = _operands(eng, Cin, csplit, proj, Hi, Wi)
    y, y2, a = _run(eng, 1, x, wt2, inv_t, b, csplit, proj, relu, am)
    r1 = F.conv2d(x.double(), w.double(), b[:csplit].double(), 2, 1)
    if relu:
        r1 = torch.relu(r1)
    assert y.shape == r1.shape
    e1, s1 = float((y.double() - r1).abs().max()), float(r1.abs().max())
    print('\n  %d -> %d%s %dx%d: y %.3e of scale' % (Cin, csplit, '+%d' % csplit if proj else '', Hi, Wi, e1 / s1), end='')
    assert e1 <= 4e-6 * s1
    if proj:
        r2 = F.conv2d(x.double(), wd.double(), b[csplit:].double(), 2, 0)
        assert y2.shape == r2.shape
        e2, s2 = float((y2.double() - r2).abs().max()), float(r2.abs().max())
        print(', y2 %.3e' % (e2 / s2), end='')
        assert e2 <= 4e-6 * s2
    assert float(a.view(torch.float32)) == float(y.abs().max())


@pytest.mark.parametrize('Cin,csplit,proj,relu', FORMS)
def test_last_image_alone_has_the_bits_it_has_in_the_batch(eng, Cin, csplit, proj, relu):
    """persistent workgroups: which workgroup computes a tile, and what it computed before, must not change a bit"""
    Hi, Wi = MANY
    nb = 3
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert _tiles(Cin, Hi, Wi, nb) > 2 * n_cu
    x, w, wd, b, wt2, inv_t, am = _operands(eng, Cin, csplit, proj, Hi, Wi, nb=nb)
    y, y2, _ = _run(eng, 1, x, wt2, inv_t, b, csplit, proj, relu, am)
    z, z2, _ = _run(eng, 1, x[nb - 1:], wt2, inv_t, b, csplit, proj, relu, am)
    _same_bits(y[nb - 1:], z, 'y')
    if proj:
        _same_bits(y2[nb - 1:], z2, 'y2')
