"""CPU self-check of tests/segnet_exact.py, the exact-operand cases behind test_gpu_segnet_exact.py: every case meets the bound
its exactness rests on; the per-tap float64 reference is torch's float64 convolution / autograd on the small shapes; the two
conv1 premises hold in float32 and float64; the kernels' float32 arithmetic restated in torch (bf16 rounding of the operands, the
three split-plane products in separate accumulators, conv1's 7 K steps of 8 taps x 4 channels with taps 49..55 zero, wgrad's chunk
partials summed in float64 and rounded once) gives the reference bit for bit; and `check` rejects that restatement with each of the
mistakes the tolerance tests cannot see."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact as ce  # noqa: E402
import segnet_exact as se  # noqa: E402

torch = pytest.importorskip('torch')
F = torch.nn.functional

SMALL1 = (1, 16, 32)                   # conv1
SMALL = (3, 6, 10)                     # the 64-channel forms: a partial tile on both axes
TWO_TILES = (1, 16, 48)                # two tile rows, two tile columns


def nchw(a):
    return a.permute(0, 3, 1, 2).contiguous()


def nhwc(a):
    return a.permute(0, 2, 3, 1).contiguous()


def bf16(t):
    return t.to(torch.bfloat16).float()


# ---------------------------------------------------------------------------------------------------- the restatement
def conv1_k_steps(x, w, tap48=True, fourth=False):
    """the bf16 conv1 K loop: x (B,H,W,3) float32 operand, w (64,3,7,7) -> (B,H,W,64) float32 accumulated over 7 steps of
    K = 32 = 8 taps x 4 channels, taps 49..55 zero.  tap48 False: the lone tap of the last step is missing.  fourth: slot 3 of
    every tap holds channel 0 in both operands instead of zero."""
    B, H, W, _ = x.shape
    x4 = F.pad(nchw(x), (0, 0, 0, 0, 0, 1))
    w4 = F.pad(w, (0, 0, 0, 0, 0, 1))
    if fourth:
        x4[:, 3], w4[:, 3] = x4[:, 0], w4[:, 0]
    pat = F.unfold(x4, 7, padding=3).view(B, 4, 49, H * W).permute(0, 3, 2, 1)           # (B, HW, tap, c)
    pat = F.pad(pat, (0, 0, 0, 7)).reshape(B, H * W, 7, 32)
    wk = w4.permute(0, 2, 3, 1).reshape(64, 49, 4).clone()
    if not tap48:
        wk[:, 48] = 0
    wk = F.pad(wk, (0, 0, 0, 7)).reshape(64, 7, 32)
    acc = torch.zeros((B, H * W, 64), dtype=torch.float32)
    for s in range(7):
        acc = acc + pat[:, :, s] @ wk[:, s].t()
    return acc.view(B, H, W, 64)


def restate(c, family, drop=None, rotate=True, transposed=False, halo=False, tap48=True, fourth=False):
    """the float32 sums of Conv c as family's kernels compute them, on the CPU, with the mutants as switches.
    drop = (channel, ky, kx): that term missing from every output; rotate False: dgrad without the 180-degree rotation; transposed:
    the unpool reads the index transposed; halo: tile (0, 0) of image 0 takes the halo pixel (2, 33) from (2, 1), the same position
    of the neighbouring tile; tap48 / fourth: conv1_k_steps'"""
    x = c.operand64(transposed=transposed).float()                                       # exact: (B,H,W,C)
    w = c.w.clone()
    if drop is not None:
        w[:, drop[0], drop[1], drop[2]] = 0
    if c.form == 'dgrad':
        w = (w.flip(2, 3) if rotate else w).transpose(0, 1).contiguous()

    def convolve(a, b):
        if c.form == 'conv1' and family == '_bf16':
            return conv1_k_steps(a, b, tap48, fourth)
        y = F.conv2d(nchw(a), b, padding=3)                                              # float32 accumulation
        if halo:
            a2 = a.clone()
            a2[0, 2, 33] = a[0, 2, 1]
            y[0, :, :se.TH, :se.TW] = F.conv2d(nchw(a2[:1]), b, padding=3)[0, :, :se.TH, :se.TW]
        return nhwc(y)
    if family == '_f16x3':
        hx, lx, sx = ce.split(x)
        hw, lw, sw = ce.split(w)
        cross = convolve(hx, lw) + convolve(lx, hw)                                      # (l l is dropped by design)
        y = (convolve(hx, hw) + cross) * torch.tensor(1.0 / (sx * sw), dtype=torch.float32)
    elif family == '_bf16':
        y = convolve(bf16(x), bf16(w))
    else:
        y = convolve(x, w)
    assert y.dtype == torch.float32
    return y


def restate_wgrad(c, family, skip_chunk=None):
    """wgrad as the kernels compute it: float32 partials per chunk of 2 x 32 tiles, the chunks summed in float64 and rounded once"""
    B, H, W = c.shape
    tiles, nch = c.chunks()
    txn = (W + se.WG_TW - 1) // se.WG_TW
    b, y, x = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing='ij')
    tile = (b * (H // se.WG_TR) + y // se.WG_TR) * txn + x // se.WG_TW
    dy, xin = c.dy, c.operand64().float()
    if family == '_bf16':
        dy, xin = bf16(dy), bf16(xin)
    total = torch.zeros((49, 64, xin.shape[3]), dtype=torch.float64)
    for j in range(nch):
        if j == skip_chunk:
            continue
        own = ((tile >= tiles * j // nch) & (tile < tiles * (j + 1) // nch)).float()[..., None]
        if family == '_f16x3':
            hg, lg, sg = ce.split(dy)
            hx, lx, sx = ce.split(xin)
            part = (se.wgrad_taps(hg * own, hx) + (se.wgrad_taps(hg * own, lx) + se.wgrad_taps(lg * own, hx))) / (sg * sx)
        else:
            part = se.wgrad_taps(dy * own, xin)
        assert part.dtype == torch.float32
        total += part.double()
    return total.float()


# ---------------------------------------------------------------------------------------------------- bounds and conditions
def test_every_gpu_case_meets_its_bound():
    """every case of the GPU file: the bound its regime's ranges give whatever the draw, and below the beyond-chip sizes (whose
    operands the GPU file makes, with the same assertions in the constructor) the operands themselves"""
    n = 0
    for form, regime, shape in se.conv_keys():
        assert se.worst_bound(form, regime) < se.LIMIT
        n += 1
        if shape in se.BEYOND_CHIP:
            continue
        c = se.Conv(form, regime, shape)
        assert c.bound <= se.worst_bound(form, regime)
        units = c.x / c.xu
        assert torch.equal(units, units.round()) and torch.equal(c.w, c.w.round())
        if regime in ('wide', 'dec1'):
            assert c.K == 3136 and 7 * 3 * c.K + 8 < se.LIMIT and float(units.max()) == 7 and float(units.min()) == 0
        if regime.startswith('planes'):
            assert (se.BIG + 2) * 1 * c.K + 16 < se.LIMIT
    for form, shapes in se.WGRAD_SHAPES.items():
        for shape in shapes:
            B, H, W = shape
            assert B * H * W * 3 < se.LIMIT
            assert shape in se.BEYOND_CHIP or se.Wgrad(form, shape).bound == B * H * W * 3
            n += 1
    assert n == len(se.conv_keys()) + 6
    # every entry point of every family at every applicable shape in each of its regimes
    assert len(se.forward_cases()) == 3 * 3 * (2 + 2 + 2) + 3 * 1 + 3 * 2 * 2
    assert len(se.dgrad_cases()) == len(se.decode_cases()) == 3 * (3 + 2)
    assert len(se.encode_cases()) == 3 * (3 + 3) + 3 + 3 * 2 and len(se.wgrad_cases()) == 18 and len(se.decode1_cases()) == 9


def test_shapes_are_edges_and_beyond_the_chip():
    assert se.workgroups((2, 256, 512)) == 1024 and se.workgroups((3, 176, 528)) == 1122
    assert all(se.workgroups(s) >= 4 * 256 for s in se.BEYOND_CHIP)
    assert se.workgroups((1, 16, 32)) == 2 and se.workgroups((3, 6, 10)) == 3
    assert 528 % se.TW == 16 and 178 % se.TH == 2 and 530 % se.TW == 18
    assert se.Wgrad('enc', (2, 6, 10)).chunks() == (6, 6) and se.Wgrad('enc', (2, 256, 512)).chunks() == (4096, 96)


def test_only_the_open_bf16_conv1_cases_may_be_marked():
    allowed = {(t, s) for t in ('forward-_bf16-conv1', 'encode-_bf16-conv1', 'identity-_bf16')
               for s in se.BEYOND_CHIP if s[1] % 16 == 0}
    assert set(se.MARKED) <= allowed
    for (test, shape), reason in se.MARKED.items():
        assert [m.name for m in se.marks(test, shape)] == ['xfail'] and reason
    assert se.marks('forward--conv1', (2, 256, 512)) == [] and se.marks('forward-_bf16-enc', (2, 256, 512)) == []


@pytest.mark.parametrize('regime', ['wide', 'stats', 'planes_x', 'planes_w'])
def test_reference_conditions_on_the_small_shapes(regime):
    """what the regimes promise about the REFERENCE: exact float32, per-tile sums (stats), both signs at the ReLU, frequent ties"""
    c = se.conv('enc', regime, SMALL)
    y = c.y()
    assert y.dtype == torch.float32 and torch.equal(y, y.round())
    if regime == 'stats':
        s = c.stats()
        assert torch.equal(s[0], y.double().sum((0, 1, 2))) and float(s[1].max()) < se.LIMIT
    else:
        pooled, idx = c.encoded()
        assert bool((c.biased() < 0).any()) and bool((pooled > 0).any())
        if regime == 'wide':
            assert c.tie_fraction() > 0.1                    # the ReLU holds half of the outputs at zero: ties are frequent
            assert len(set(idx.reshape(-1).tolist())) == 4


# ---------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('form,regime,shape', [('enc', 'wide', SMALL), ('dec', 'wide', SMALL), ('dec', 'planes_x', SMALL),
                                                ('conv1', 'tiny', SMALL1), ('conv1', 'stats', SMALL1)])
def test_per_tap_reference_is_the_float64_convolution(form, regime, shape):
    c = se.conv(form, regime, shape)
    x = c.operand64()
    if form == 'dec':
        B, H, W = shape
        ref_unpooled = torch.zeros_like(x)
        for b, y, xx, ch in itertools.product(range(B), range(H // 2), range(W // 2), range(0, 64, 13)):
            r = int(c.idx[b, y, xx, ch])
            ref_unpooled[b, 2 * y + (r >> 1), 2 * xx + (r & 1), ch] = c.x[b, y, xx, ch]
        assert torch.equal(x[..., ::13], ref_unpooled[..., ::13])
    ref = nhwc(F.conv2d(nchw(x), c.w.double(), padding=3))
    assert torch.equal(c.y().double(), ref)


def test_per_tap_dgrad_and_wgrad_are_float64_autograd():
    c = se.conv('dgrad', 'wide', SMALL)
    dy = nchw(c.operand64())
    x = torch.zeros_like(dy, requires_grad=True)
    F.conv2d(x, c.w.double(), padding=3).backward(dy)
    assert torch.equal(c.y().double(), nhwc(x.grad))
    h = torch.zeros((3, 3, 5, 64), dtype=torch.float64, requires_grad=True)
    F.conv2d(nchw(se.unpool(h, c.idx)), c.w.double(), padding=3).backward(dy)
    assert torch.equal(c.pooled_grad().double(), h.grad)
    for form, shape in (('enc', (2, 6, 10)), ('dec', (2, 6, 10)), ('conv1', SMALL1)):
        g = se.wgrad(form, shape)
        w = torch.zeros((64, g.operand64().shape[3], 7, 7), dtype=torch.float64, requires_grad=True)
        F.conv2d(nchw(g.operand64()), w, padding=3).backward(nchw(g.dy.double()))
        assert torch.equal(se.pack_weight(w.grad), g.dw().double())
        if form == 'conv1':
            assert not bool(g.dw()[:, :, 3].any())


def test_first_maximum_and_unpool_agree_with_the_plain_loops():
    c = se.conv('enc', 'wide', SMALL)
    v = torch.relu(c.biased())
    pooled, idx = c.encoded()
    for b, y, x, ch in itertools.product(range(3), range(3), range(5), range(0, 64, 7)):
        win = [float(v[b, 2 * y + (r >> 1), 2 * x + (r & 1), ch]) for r in range(4)]
        assert float(pooled[b, y, x, ch]) == max(win) and int(idx[b, y, x, ch]) == win.index(max(win))
    assert torch.equal(se.gather_pooled(se.unpool(pooled, idx), idx), pooled)


# ---------------------------------------------------------------------------------------------------- the conv1 premises
def test_tiny_pixels_pass_the_float32_lrn_unchanged():
    """all 33^3 triples: 1.f + alpha s is 1.f in float32 (largest |1 + alpha s - 1| is 0), so the operand is the pixel"""
    k = torch.arange(-16, 17, dtype=torch.float32) * se.TINY_UNIT
    t = torch.cartesian_prod(k, k, k)
    a2, b2, c2 = (t * t).unbind(1)
    alpha = torch.tensor(1e-4, dtype=torch.float32) / 5
    for s in ((a2 + b2) + c2, (b2 + a2) + c2, (c2 + b2) + a2):                           # sg_lrn3's three orders
        one = 1.0 + alpha * s
        assert one.dtype == torch.float32 and float((one - 1.0).abs().max()) == 0.0
        assert torch.equal(t[:, 0] * torch.pow(one, -0.75), t[:, 0])
    assert se.ALPHA * float(((t.double() ** 2).sum(1)).max()) < 1.47e-8 < 2.0 ** -25


def test_integer_pixels_round_to_themselves_in_bf16_with_a_margin():
    """all 11^3 triples in -5..5: the exact operand's bf16 rounding is the pixel, the nearest rounding boundary >= 16 000 float32
    ulps away; the float32 restatement of the LRN agrees.  At |x| <= 7 the margin is below 1000 ulps: the regime stops at 5."""
    def triples(n):
        k = torch.arange(-n, n + 1, dtype=torch.float32)
        return torch.cartesian_prod(k, k, k).view(-1, 3, 1, 1)
    t = triples(5)
    m = float(se.bf16_margin_ulps(t, se.lrn64(t)).min())
    print('margin at |x| <= 5: %.0f float32 ulps' % m)
    assert 16000 <= m <= 16400
    s = (t * t).sum(1, keepdim=True)
    v32 = t * torch.pow(1.0 + torch.tensor(se.ALPHA, dtype=torch.float32) * s, -0.75)
    assert v32.dtype == torch.float32 and torch.equal(bf16(v32), t) and not torch.equal(v32, t)
    assert float((v32.double() - se.lrn64(t)).abs().max()) < 1e-6                         # far inside the margin
    t7 = triples(7)
    m7 = float(se.bf16_margin_ulps(t7, se.lrn64(t7)).min())
    print('margin at |x| <= 7: %.0f float32 ulps' % m7)
    assert 0 < m7 < 1000
    assert se.conv('conv1', 'ints', SMALL1).margin >= 16000


# ---------------------------------------------------------------------------------------------------- restatement and mutants
FORMS = [('enc', 'wide', SMALL), ('dec', 'wide', SMALL), ('dgrad', 'wide', SMALL), ('enc', 'stats', SMALL),
         ('conv1', 'tiny', SMALL1), ('conv1', 'stats', SMALL1)]


@pytest.mark.parametrize('family', se.FAMILIES)
@pytest.mark.parametrize('form,regime,shape', FORMS + [('enc', 'planes_x', SMALL), ('dec', 'planes_w', SMALL),
                                                       ('dgrad', 'planes_x', SMALL), ('conv1', 'ints', SMALL1)])
def test_restated_float32_arithmetic_is_the_reference_bit_for_bit(family, form, regime, shape):
    if regime.startswith('planes') and family != '_f16x3' or regime == 'ints' and family != '_bf16':
        return                                                     # (the GPU file has no such case either)
    c = se.conv(form, regime, shape)
    se.check(restate(c, family), c.y(), 'restatement')


@pytest.mark.parametrize('family', se.FAMILIES)
@pytest.mark.parametrize('form,shape', [('enc', (2, 6, 10)), ('dec', (2, 6, 10)), ('conv1', SMALL1)])
def test_restated_wgrad_is_the_reference_bit_for_bit(family, form, shape):
    g = se.wgrad(form, shape)
    se.check(restate_wgrad(g, family), g.dw(), 'wgrad restatement')


def rejected(y, ref, what):
    with pytest.raises(AssertionError, match='outputs differ'):
        se.check(y, ref, what)


@pytest.mark.parametrize('family', se.FAMILIES)
def test_check_rejects_every_mutant_of_the_64_channel_forms(family):
    enc, dec, dg = (se.conv(f, 'wide', SMALL) for f in ('enc', 'dec', 'dgrad'))
    rejected(restate(enc, family, drop=(37, 0, 5)), enc.y(), 'one (tap, channel) term of K = 3136 dropped')
    rejected(restate(dec, family, transposed=True), dec.y(), 'the unpool selects the wrong position of a window')
    rejected(restate(dg, family, rotate=False), dg.y(), 'dgrad without the 180-degree rotation')
    two = se.conv('enc', 'wide', TWO_TILES)
    se.check(restate(two, family), two.y())
    rejected(restate(two, family, halo=True), two.y(), 'a halo pixel from the neighbouring tile\'s position')
    v = torch.relu(restate(enc, family) + enc.bias)
    pooled, idx = enc.encoded()
    se.check(se.pool_first(v)[0], pooled)
    se.check(se.pool_first(v)[1], idx)
    se.check(se.pool_first(v, last=True)[0], pooled)               # the value is the same: only the index tells
    rejected(se.pool_first(v, last=True)[1], idx, 'last maximum instead of first')
    rejected(se.gather_pooled(dg.y(), dg.idx ^ 1), dg.pooled_grad(), 'the pooled gradient gathered at the wrong position')
    g = se.wgrad('enc', (2, 6, 10))
    rejected(restate_wgrad(g, family, skip_chunk=4), g.dw(), 'one wgrad chunk left out of the sum')


@pytest.mark.parametrize('regime', ['tiny', 'ints'])
def test_check_rejects_every_mutant_of_conv1(regime):
    c = se.conv('conv1', regime, SMALL1)
    se.check(restate(c, '_bf16'), c.y())
    rejected(restate(c, '_bf16', tap48=False), c.y(), 'tap 48, the lone tap of the last K step, dropped')
    rejected(restate(c, '_bf16', fourth=True), c.y(), 'a non-zero fourth channel')
    rejected(restate(c, '', drop=(2, 6, 6)), c.y(), 'one of 147 terms dropped')
    g = se.wgrad('conv1', SMALL1)
    dw = g.dw().clone()
    dw[:, :, 3] = dw[:, :, 0]
    rejected(dw, g.dw(), 'a non-zero fourth channel of conv1\'s weight gradient')


def test_planes_regimes_need_the_low_plane():
    for regime in ('planes_x', 'planes_w'):
        c = se.conv('enc', regime, SMALL)
        hx, lx, sx = ce.split(c.operand64().float())
        hw, lw, sw = ce.split(c.w)
        y = nhwc(F.conv2d(nchw(hx), hw, padding=3)) * torch.tensor(1.0 / (sx * sw), dtype=torch.float32)
        rejected(y, c.y(), 'low plane zeroed')


def test_check_reports_the_first_difference():
    c = se.conv('enc', 'wide', SMALL)
    y = c.y().clone()
    y[1, 3, 2, 7] += 1
    y[2, 0, 0, 9] += 1
    with pytest.raises(AssertionError) as e:
        se.check(y, c.y(), 'probe')
    assert 'probe: 2 of %d outputs differ' % y.numel() in str(e.value) and '(1, 3, 2, 7)' in str(e.value)
    with pytest.raises(AssertionError):
        se.check(c.y().double(), c.y())
