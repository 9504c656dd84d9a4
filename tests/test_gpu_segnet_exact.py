"""GPU tests of the SegNet 7x7 kernels (csrc/spa_segnet*.hip without spa_segnet_input.hip) on operands whose result is known bit
for bit, at grids beyond the chip (tests/segnet_exact.py has the argument, the regimes and the premise).  Every entry point of the
three families (float32, bf16, split f16 planes) runs in each of its regimes at an edge shape and at two shapes of >= 4 workgroups
per CU (asserted from the device's CU count), into NaN- / 255-poisoned outputs with a guard, twice: the result must be the float64
reference (torch.equal, no tolerance, no exempt element; decode1's probabilities within the family's PROB_TOL of the float64
softmax of the exact logits) and the second call must give the same bits.  The float64 reference is computed on the device, once
per (form, regime, shape).  The conv1 premise (the float32 kernel's operand is the image on these operands) is tested first; the
identity-weight tests at the end localise a difference of the bf16 conv1 kernels: operand or accumulation, and where in the tile."""
import ctypes
import importlib
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_exact as se  # noqa: E402
import segnet_ref as sref  # noqa: E402

segnet = importlib.import_module('superpixel-align_amd.segnet')

# decode1's probabilities, absolute: PROB_TOL of test_gpu_segnet.py, test_gpu_segnet_bf16.py and test_gpu_segnet_f16x3.py
PROB_TOL = {'': 1e-5, '_bf16': 1e-5, '_f16x3': 1e-5}
NHWC, NCHW = 0, 1


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()
    se.conv.cache_clear()                    # the operands and device references of this file: a few GB
    se.wgrad.cache_clear()
    torch.cuda.empty_cache()


def beyond(shape):
    """a beyond-chip shape is >= 4 workgroups per CU on THIS device: a different part fails loudly instead of testing less"""
    if tuple(shape) in se.BEYOND_CHIP:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert se.workgroups(shape) >= 4 * cus, '%s is %d workgroups for %d CUs' % (shape, se.workgroups(shape), cus)


def dev(t):
    return None if t is None else t.cuda().contiguous()


def std_of(c):
    return (se.ZERO3, se.ONE3) if c.form == 'conv1' else (None, None)


def params(cases, test):
    """pytest params of (family, [form,] [regime,] shape) cases; a case's marks are segnet_exact.MARKED's, nothing else"""
    out = []
    for k in cases:
        form = next((v for v in k[1:] if v in ('conv1', 'enc', 'dec')), '')
        name = '%s-%s-%s' % (test, k[0], form) if form else '%s-%s' % (test, k[0])
        ident = '-'.join('x'.join(map(str, v)) if isinstance(v, tuple) else (v or 'f32') for v in k)
        out.append(pytest.param(*k, marks=se.marks(name, k[-1]), id=ident))
    return out


def identity_weight():
    w = torch.zeros((64, 3, 7, 7))
    for ch in range(3):
        w[ch, ch, 3, 3] = 1.0
    return dev(se.pack_weight(w))


def forward_twice(eng, family, c, wt=None, stats=False):
    """the training forward of Conv c into poisoned outputs, twice -> [(y, stats), (y, stats)]"""
    B, H, W = c.shape
    fwd = getattr(eng, 'segnet_train_forward' + family)
    x, idx, wt = dev(c.x), dev(c.idx), dev(c.wt()) if wt is None else wt
    mean, std = std_of(c)
    runs = []
    for rep in range(2):
        out, buf = sref.poisoned((B, H, W, 64))
        y, s = fwd(x, wt, idx, mean, std, stats=stats, out=out)
        torch.cuda.synchronize()
        sref.check_guard(buf, B * H * W * 64)
        runs.append((y, s))
    assert eng.status() == 0
    return runs


# ---------------------------------------------------------------------------------------------------- the premise, first
@pytest.mark.parametrize('shape', se.CONV1_SHAPES, ids=str)
@pytest.mark.parametrize('regime', ['tiny', 'ints', 'stats'])
def test_premise_float32_conv1_operand_is_the_image(eng, regime, shape):
    """PREMISE of the conv1 regimes: through the float32 training forward a centre-tap identity weight returns the operand the
    kernels multiply.  'tiny' / 'stats': it is the image bit for bit (LRN is the identity).  'ints': its bf16 rounding is."""
    beyond(shape)
    c = se.conv('conv1', regime, shape)
    (y, _), (y2, _) = forward_twice(eng, '', c, wt=identity_weight())
    assert torch.equal(y, y2)
    img = dev(c.x.permute(0, 2, 3, 1))
    assert not bool(y[..., 3:].any())
    if regime == 'ints':
        assert not torch.equal(y[..., :3], img), 'LRN is meant to be active'
        se.check(y[..., :3].to(torch.bfloat16).float(), img, 'bf16 rounding of the float32 operand')
        m = float(se.bf16_margin_ulps(img, y[..., :3]).min())
        print('ints %s: the float32 operand is >= %.0f float32 ulps from a bf16 rounding boundary' % (shape, m))
        assert m >= 1000
    else:
        se.check(y[..., :3].contiguous(), img, 'the float32 operand')


# ---------------------------------------------------------------------------------------------------- training
@pytest.mark.parametrize('family,form,regime,shape', params(se.forward_cases(), 'forward'))
def test_train_forward_is_exact(eng, family, form, regime, shape):
    beyond(shape)
    c = se.conv(form, regime, shape)
    what = 'segnet_train_forward%s %s %s %s' % (family, form, regime, shape)
    (y, s), (y2, s2) = forward_twice(eng, family, c, stats=regime == 'stats')
    se.check(y, c.y('cuda'), what)
    assert torch.equal(y, y2), what + ': the second call differs'
    if regime == 'stats':
        assert torch.equal(s, c.stats('cuda')), what + ': (sum y, sum y^2)'
        assert torch.equal(s, s2)


@pytest.mark.parametrize('family,regime,shape', params(se.dgrad_cases(), 'dgrad'))
def test_train_dgrad_is_exact(eng, family, regime, shape):
    beyond(shape)
    B, H, W = shape
    c = se.conv('dgrad', regime, shape)
    dgrad = getattr(eng, 'segnet_train_dgrad' + family)
    dy, wt, idx = dev(c.x), dev(c.wt()), dev(c.idx)
    for ii, ref, n in ((None, c.y('cuda'), (B, H, W, 64)), (idx, c.pooled_grad('cuda'), (B, H // 2, W // 2, 64))):
        what = 'segnet_train_dgrad%s %s %s %s' % (family, 'pooled' if ii is not None else 'plain', regime, shape)
        got = []
        for rep in range(2):
            out, buf = sref.poisoned(n)
            got.append(dgrad(dy, wt, ii, out=out))
            torch.cuda.synchronize()
            sref.check_guard(buf, out.numel())
        se.check(got[0], ref, what)
        assert torch.equal(got[0], got[1]), what + ': the second call differs'
    assert eng.status() == 0


@pytest.mark.parametrize('family,form,shape', params(se.wgrad_cases(), 'wgrad'))
def test_train_wgrad_is_exact(eng, family, form, shape):
    g = se.wgrad(form, shape)
    wgrad = getattr(eng, 'segnet_train_wgrad' + family)
    dy, x, idx = dev(g.dy), dev(g.x), dev(g.idx)
    mean, std = std_of(g)
    cp = 4 if form == 'conv1' else 64
    what = 'segnet_train_wgrad%s %s %s (%d tiles in %d chunks)' % ((family, form, shape) + g.chunks())
    got = []
    for rep in range(2):
        out, buf = sref.poisoned((49, 64, cp))
        got.append(wgrad(dy, x, idx, mean, std, out=out))
        torch.cuda.synchronize()
        sref.check_guard(buf, 49 * 64 * cp)
    se.check(got[0], g.dw('cuda'), what)
    assert torch.equal(got[0], got[1]), what + ': the second call differs'
    assert eng.status() == 0


# ---------------------------------------------------------------------------------------------------- inference
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def poisoned_u8(shape):
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + 1024,), 255, dtype=torch.uint8, device='cuda')
    return buf[:n].view(shape), buf


def encode_twice(eng, family, form, shape, x, wt, bias, mean=se.ZERO3, std=se.ONE3):
    """spa_segnet_encode* through the C entry point into poisoned outputs, twice -> [(pooled, idx)], each (B,H/2,W/2,64)"""
    B, H, W = shape
    enc = getattr(eng._lib, 'spa_segnet_encode' + family)
    x, wt, bias = dev(x), dev(wt), dev(bias)
    runs = []
    for rep in range(2):
        out, buf = sref.poisoned((B, H // 2, W // 2, 64))
        oi, ibuf = poisoned_u8((B, H // 2, W // 2, 64))
        if form == 'conv1':
            rc = enc(eng._ctx, _p(x), NCHW, B, H, W, 3, _p(wt), _p(bias), (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std),
                     _p(out), _p(oi), _stream())
        else:
            rc = enc(eng._ctx, _p(x), NHWC, B, H, W, 64, _p(wt), _p(bias), None, None, _p(out), _p(oi), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        sref.check_guard(buf, out.numel())
        assert bool((ibuf[oi.numel():] == 255).all()), 'a kernel wrote past the end of its index map'
        runs.append((out, oi))
    assert eng.status() == 0
    return runs


@pytest.mark.parametrize('family,form,regime,shape', params(se.encode_cases(), 'encode'))
def test_encode_is_exact(eng, family, form, regime, shape):
    """pooled values AND the first-maximum index of every window: equal values inside a window are frequent and exact here"""
    beyond(shape)
    c = se.conv(form, regime, shape)
    what = 'segnet_encode%s %s %s %s' % (family, form, regime, shape)
    (pooled, idx), (pooled2, idx2) = encode_twice(eng, family, form, shape, c.x, c.wt(), c.bias)
    ref, ref_idx = c.encoded('cuda')
    se.check(pooled, ref, what)
    se.check(idx, ref_idx, what + ' index')
    assert torch.equal(pooled, pooled2) and torch.equal(idx, idx2), what + ': the second call differs'


def decode_twice(eng, family, c, classifier):
    B, H, W = c.shape
    dec = getattr(eng._lib, 'spa_segnet_decode' + family)
    h, idx, wt, bias = dev(c.x), dev(c.idx), dev(c.wt()), dev(c.bias)
    wc, bc = (dev(c.wc), dev(c.bc)) if classifier else (None, None)
    got = []
    for rep in range(2):
        out, buf = sref.poisoned((B, 2, H, W) if classifier else (B, H, W, 64))
        rc = dec(eng._ctx, _p(h), _p(idx), NHWC, B, H // 2, W // 2, _p(wt), _p(bias), _p(wc), _p(bc), _p(out), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        sref.check_guard(buf, out.numel())
        got.append(out)
    assert eng.status() == 0
    return got


@pytest.mark.parametrize('family,regime,shape', params(se.decode_cases(), 'decode'))
def test_decode_is_exact(eng, family, regime, shape):
    beyond(shape)
    c = se.conv('dec', regime, shape)
    what = 'segnet_decode%s %s %s' % (family, regime, shape)
    y, y2 = decode_twice(eng, family, c, False)
    se.check(y, c.biased('cuda'), what)
    assert torch.equal(y, y2), what + ': the second call differs'


@pytest.mark.parametrize('family,shape', params(se.decode1_cases(), 'decode1'))
def test_decode1_probabilities_of_exact_logits(eng, family, shape):
    """the logits are exact; the softmax is not: within PROB_TOL of the float64 softmax of the exact logits, and repeatable"""
    beyond(shape)
    c = se.conv('dec', 'dec1', shape)
    p, p2 = decode_twice(eng, family, c, True)
    z = c.logits64('cuda')
    gap = (z[:, 0] - z[:, 1]).abs()
    assert float((gap < 8).double().mean()) > 0.5 and float(gap.max()) > 1, 'the softmax is meant to be neither saturated nor flat'
    err = float((p.double() - torch.softmax(z, 1)).abs().max())
    print('segnet_decode%s decode1 %s: probability error %.3g' % (family, shape, err))
    assert err <= PROB_TOL[family]
    assert torch.equal(p, p2)


# ---------------------------------------------------------------------------------------------------- localising a bf16 conv1 difference
def _tile_positions(mask):
    """(count, the most frequent (row mod 8, column mod 32) positions) of the set pixels of a (B,H,W) mask"""
    b, y, x = mask.nonzero(as_tuple=True)
    pos, cnt = torch.unique((y % se.TH) * se.TW + x % se.TW, return_counts=True)
    top = sorted(zip(cnt.tolist(), pos.tolist()), reverse=True)[:8]
    return int(mask.sum()), ['(%d,%d)x%d' % (p // se.TW, p % se.TW, n) for n, p in top]


def _describe(a, b, x32, what):
    """a, b: (B,H,W,3) bf16 operands (as float32) of two calls; x32 the float32 kernel's operand"""
    r = x32.to(torch.bfloat16).float()
    lines = []
    for name, u, v in (('call 2 differs from call 1', a, b), ('call 1 differs from bf16(float32 operand)', a, r)):
        d = u != v
        if not bool(d.any()):
            lines.append('%s: %s: nowhere' % (what, name))
            continue
        n, top = _tile_positions(d.any(-1))
        step = torch.maximum(u.abs(), v.abs())[d].to(torch.bfloat16)
        one = ((u[d] - v[d]).abs() <= (step.view(torch.int16) + 1).view(torch.bfloat16).float() - step.float())
        margin = se.bf16_margin_ulps(r[d], x32[d])
        lines.append('%s: %s: %d pixels, %d values; tile positions (row, col) x count: %s; one bf16 step: %d of %d; distance of '
                     'the float32 operand to a bf16 boundary: min %.1f median %.1f max %.1f float32 ulps'
                     % (what, name, n, int(d.sum()), ' '.join(top), int(one.sum()), one.numel(), float(margin.min()),
                        float(margin.median()), float(margin.max())))
    return '\n'.join(lines)


IDENTITY_SHAPE = (2, 256, 512)


@pytest.mark.parametrize('image', ['tiny', 'ints', 'seeded'])
@pytest.mark.parametrize('family,shape', params([('_bf16', IDENTITY_SHAPE)], 'identity'))
def test_bf16_conv1_operand_through_the_identity_weight(eng, family, shape, image):
    """The centre-tap identity weight returns the bf16 operand per pixel (one product per output) through the bf16 forward, and its
    2x2 maximum through segnet_encode_bf16.  Each is called twice.  The two calls must agree, and the operand must be the bf16
    rounding of the float32 kernel's operand bit for bit (spa_segnet_dev.h: both get the value from the same function): the image
    itself on the exact images, and on a seeded 0..255 image with the dataset's mean and std, where the LRN's powf is at work.
    On a difference the message gives the count, the positions modulo the tile, the distance of the float32 operand to a bf16
    rounding boundary and whether the difference is one bf16 step: 'the float32 LRN value is not stable' (one step, near a
    boundary, anywhere in the tile) against 'staging or K loop reads something else'."""
    beyond(shape)
    B, H, W = shape
    wid = identity_weight()
    if image == 'seeded':
        img = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(7)) * 255.0
        mean, std = tuple(segnet.MEAN), tuple(segnet.STD)
    else:
        img, mean, std = se.conv('conv1', image, shape).x, se.ZERO3, se.ONE3
    x = dev(img)
    ops = {}
    for fam in ('', '_bf16'):
        fwd = getattr(eng, 'segnet_train_forward' + fam)
        ops[fam] = [fwd(x, wid, None, mean, std, stats=False)[0][..., :3].contiguous() for rep in range(2)]
    torch.cuda.synchronize()
    x32, x32b = ops['']
    a, b = ops['_bf16']
    assert torch.equal(x32, x32b), 'the float32 control is not repeatable'
    report = _describe(a, b, x32, 'forward_bf16 %s %s' % (image, shape))
    (p1, i1), (p2, i2) = encode_twice(eng, '_bf16', 'conv1', shape, x, wid, torch.zeros(64), mean, std)
    want = se.pool_first(torch.relu(a))
    dp = (p1[..., :3] != p2[..., :3])
    report += '\nencode_bf16 %s %s: call 2 differs from call 1 at %d pooled values; call 1 differs from the pooled forward operand ' \
              'at %d' % (image, shape, int(dp.sum()), int((p1[..., :3] != want[0]).sum()))
    print(report)
    assert torch.equal(a, b) and torch.equal(p1, p2) and torch.equal(i1, i2), report
    if image != 'seeded':
        se.check(a, dev(img.permute(0, 2, 3, 1)), 'the bf16 operand of the %s image\n%s' % (image, report))
    se.check(a, x32.to(torch.bfloat16).float(), 'the bf16 operand against bf16(float32 operand)\n' + report)
    se.check(p1[..., :3].contiguous(), want[0], 'encode_bf16 against the pooled forward operand\n' + report)
    se.check(i1[..., :3].contiguous(), want[1], 'encode_bf16 index')
