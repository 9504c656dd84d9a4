"""GPU tests of SegNet-Basic training at float32 accuracy on the f16 matrix cores (csrc/spa_segnet_train_f16x3.hip,
SegNetTrainer(..., split_planes=True), train_segnet.py --split_planes): the eight pass forms against float64 torch
convolutions of the UNROUNDED float32 operands within the float32 forms' bounds, also at extreme dynamic range, exact
zeros, the BatchNorm partial sums, NaN-poisoned outputs with a guard past the end, the float32 entry points' refusal
codes, bit-identical repeats within and across contexts, one whole step against the float64 restatement within the
float32 step's bounds, and train_segnet.py --split_planes -> --resume -> labels_from_segnet.py end to end."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
F = torch.nn.functional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
segnet = importlib.import_module('superpixel-align_amd.segnet')
st = importlib.import_module('superpixel-align_amd.segnet_train')

SHAPES = [(1, 16, 16), (2, 48, 80), (3, 64, 128), (2, 6, 10)]
# (2, 6, 10): a conv4 / decode4 resolution (1/8 of the input): a partial row tile; conv1 needs multiples of 16

# The float32 suite's bounds, as a fraction of max|ref|, against float64 products of the unrounded float32 operands.
FWD_TOL = 1e-5
WGRAD_TOL = 1e-5
WGRAD_BIG_TOL = 2e-5
BN_TOL = 1e-6

# dynamic range: inputs at 2^20, output gradients at 2^-30, weights at 2^-12 (f16 spans 2^-24 .. 2^16)
X_SCALE, DY_SCALE, W_SCALE = 2.0 ** 20, 2.0 ** -30, 2.0 ** -12


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


def poisoned(shape, dtype=torch.float32, guard=1024):
    """(out view, whole buffer): NaN everywhere, a NaN guard of `guard` elements past the end of the view"""
    n = int(np.prod(shape))
    buf = torch.full((n + guard,), float('nan'), dtype=dtype, device='cuda')
    return buf[:n].view(shape), buf


def check_guard(buf, n):
    assert torch.isnan(buf[n:]).all().item(), 'a kernel wrote past the end of its output'


def rel_err(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def d64(t):
    return t.float().double()


def inputs(B, H, W, seed, xs=1.0, dys=1.0, ws=1.0):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((B, 3, H, W), generator=g) * 255.0 * xs
    x = torch.randn((B, H, W, 64), generator=g) * xs
    h = torch.randn((B, H // 2, W // 2, 64), generator=g) * xs
    idx = torch.randint(0, 4, (B, H // 2, W // 2, 64), generator=g, dtype=torch.uint8)
    dy = torch.randn((B, H, W, 64), generator=g) * dys
    w1 = torch.randn((64, 3, 7, 7), generator=g) * (2.0 / 147) ** 0.5 * ws
    w64 = torch.randn((64, 64, 7, 7), generator=g) * (2.0 / 3136) ** 0.5 * ws
    return img, x, h, idx, dy, w1, w64


def nchw(a):
    return a.permute(0, 3, 1, 2)


def conv1_operand(eng, img):
    """conv1's float32 input exactly as the float32 kernels load it (standardised, LRN in float32): the float32
    forward pass with a centre-tap identity weight returns it (one exact product per output), (B,H,W,3) float32"""
    wid = torch.zeros((64, 3, 7, 7))
    for c in range(3):
        wid[c, c, 3, 3] = 1.0
    wt = torch.from_numpy(segnet.pack_weight(wid.numpy())).cuda()
    y, _ = eng.segnet_train_forward(img.cuda().contiguous(), wt, None, segnet.MEAN, segnet.STD, stats=False)
    return y[..., :3].cpu()


def ref_forms(eng, img, x, h, idx):
    """float64 (B,C,H,W) unrounded operands of the three input forms: conv1's image, the map, the unpooled map"""
    x1 = nchw(d64(conv1_operand(eng, img))) if img.shape[2] % 16 == 0 else None
    return x1, nchw(d64(x)), st.unpool_ref(nchw(d64(h)), nchw(idx.long()))


def check_forward(eng, shape, seed, **scales):
    B, H, W = shape
    img, x, h, idx, dy, w1, w64 = inputs(B, H, W, seed, **scales)
    x1, xe, xd = ref_forms(eng, img, x, h, idx)
    cases = [('conv1', img, None, w1, x1), ('enc', x, None, w64, xe), ('dec', h, idx, w64, xd)]
    worst = 0.0
    for name, xin, ii, w, xref in cases[1:] if H % 16 else cases:
        wt = torch.from_numpy(segnet.pack_weight(w.numpy())).cuda()
        out, buf = poisoned((B, H, W, 64))
        ii = ii.cuda() if ii is not None else None
        y, stats = eng.segnet_train_forward_f16x3(xin.cuda().contiguous(), wt, ii, segnet.MEAN, segnet.STD, out=out)
        torch.cuda.synchronize()
        check_guard(buf, B * H * W * 64)
        assert not torch.isnan(y).any().item(), '%s: an output was not stored' % name
        ref = F.conv2d(xref, d64(w), padding=3)                      # (B,64,H,W)
        e = rel_err(nchw(y), ref)
        worst = max(worst, e)
        assert e < FWD_TOL, '%s %s %s: forward error %.3g' % (name, shape, scales, e)
        # the BN partial sums are the kernel's own y summed; compare with float64 sums of that y
        y64 = y.double()
        s_ref = torch.stack([y64.sum((0, 1, 2)), (y64 * y64).sum((0, 1, 2))])
        scale = torch.stack([y64.abs().sum((0, 1, 2)), (y64 * y64).sum((0, 1, 2))])
        es = float(((stats - s_ref).abs() / scale).max())
        assert es < BN_TOL, '%s %s: BN sum error %.3g' % (name, shape, es)
        y2, stats2 = eng.segnet_train_forward_f16x3(xin.cuda().contiguous(), wt, ii, segnet.MEAN, segnet.STD)
        assert torch.equal(y2, y) and torch.equal(stats2, stats), '%s: repeat differs' % name
    return worst


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_forms_and_bn_sums(eng, shape):
    print('f16x3 forward %s: worst %.3g' % (shape, check_forward(eng, shape, 1)))


def check_dgrad(eng, shape, seed, **scales):
    B, H, W = shape
    img, x, h, idx, dy, w1, w64 = inputs(B, H, W, seed, **scales)
    wt = torch.from_numpy(segnet.pack_weight(w64.numpy())).cuda()
    dyd = dy.cuda().contiguous()
    # encoder: full-resolution input gradient
    xe = nchw(d64(x)).requires_grad_(True)
    F.conv2d(xe, d64(w64), padding=3).backward(nchw(d64(dy)))
    out, buf = poisoned((B, H, W, 64))
    dx = eng.segnet_train_dgrad_f16x3(dyd, wt, out=out)
    torch.cuda.synchronize()
    check_guard(buf, B * H * W * 64)
    assert not torch.isnan(dx).any().item()
    e1 = rel_err(nchw(dx), xe.grad)
    assert e1 < FWD_TOL, 'enc dgrad %s %s: %.3g' % (shape, scales, e1)
    assert torch.equal(eng.segnet_train_dgrad_f16x3(dyd, wt), dx)
    # decoder: the gradient at the pooled input, through the index map
    hd = nchw(d64(h)).requires_grad_(True)
    F.conv2d(st.unpool_ref(hd, nchw(idx.long())), d64(w64), padding=3).backward(nchw(d64(dy)))
    out, buf = poisoned((B, H // 2, W // 2, 64))
    dh = eng.segnet_train_dgrad_f16x3(dyd, wt, idx.cuda(), out=out)
    torch.cuda.synchronize()
    check_guard(buf, B * H * W * 16)
    assert not torch.isnan(dh).any().item()
    e2 = rel_err(nchw(dh), hd.grad)
    assert e2 < FWD_TOL, 'dec dgrad %s %s: %.3g' % (shape, scales, e2)
    assert torch.equal(eng.segnet_train_dgrad_f16x3(dyd, wt, idx.cuda()), dh)
    return max(e1, e2)


@pytest.mark.parametrize('shape', SHAPES)
def test_dgrad_forms(eng, shape):
    print('f16x3 dgrad %s: worst %.3g' % (shape, check_dgrad(eng, shape, 2)))


def wgrad_ref(dy, xin):
    """float64 on the device: dW[t][n][c] = sum_p dy[p][n] * xin[p + off(t)][c], dy (B,H,W,64), xin (B,H,W,C)"""
    B, H, W, C = xin.shape
    xp = F.pad(xin, (0, 0, 3, 3, 3, 3))
    g = dy.reshape(-1, 64)
    out = torch.empty((49, 64, C), dtype=torch.float64, device=dy.device)
    for ky in range(7):
        for kx in range(7):
            out[ky * 7 + kx] = g.t() @ xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, C)
    return out


def check_wgrad(eng, shape, seed, **scales):
    B, H, W = shape
    img, x, h, idx, dy, w1, w64 = inputs(B, H, W, seed, **scales)
    x1, xe, xd = ref_forms(eng, img, x, h, idx)
    dyd = dy.cuda().contiguous()
    dyr = d64(dy).cuda()
    cases = [('conv1', img, None, x1, 4), ('enc', x, None, xe, 64), ('dec', h, idx, xd, 64)]
    worst = 0.0
    for name, xin, ii, xref, cp in cases[1:] if H % 16 else cases:
        out, buf = poisoned((49, 64, cp))
        ii = ii.cuda() if ii is not None else None
        dw = eng.segnet_train_wgrad_f16x3(dyd, xin.cuda().contiguous(), ii, segnet.MEAN, segnet.STD, out=out)
        torch.cuda.synchronize()
        check_guard(buf, 49 * 64 * cp)
        assert not torch.isnan(dw).any().item(), '%s: an output was not stored' % name
        xr = F.pad(xref, (0, 0, 0, 0, 0, 1)) if cp == 4 else xref      # conv1: channel 3 is zero
        ref = wgrad_ref(dyr, xr.permute(0, 2, 3, 1).contiguous().cuda())
        e = rel_err(dw, ref)
        worst = max(worst, e)
        assert e < WGRAD_TOL, '%s wgrad %s %s: %.3g' % (name, shape, scales, e)
        if cp == 4:
            assert torch.equal(dw[:, :, 3], torch.zeros_like(dw[:, :, 3]))
        dw2 = eng.segnet_train_wgrad_f16x3(dyd, xin.cuda().contiguous(), ii, segnet.MEAN, segnet.STD)
        assert torch.equal(dw2, dw), '%s wgrad: repeat differs' % name
    return worst


@pytest.mark.parametrize('shape', SHAPES)
def test_wgrad_forms(eng, shape):
    print('f16x3 wgrad %s: worst %.3g' % (shape, check_wgrad(eng, shape, 3)))


def test_wgrad_decode1_full_size(eng):
    """decode1's weight gradient at B = 4, 512 x 1024: K = 2.1e6 products per output, split over the chunks"""
    B, H, W = 4, 512, 1024
    g = torch.Generator(device='cuda').manual_seed(4)
    h = torch.randn((B, H // 2, W // 2, 64), generator=g, device='cuda')
    idx = torch.randint(0, 4, (B, H // 2, W // 2, 64), generator=g, device='cuda', dtype=torch.uint8)
    dy = torch.randn((B, H, W, 64), generator=g, device='cuda')
    dw = eng.segnet_train_wgrad_f16x3(dy, h, idx)
    xd = st.unpool_ref(nchw(h.double()), nchw(idx.long())).permute(0, 2, 3, 1)
    ref = wgrad_ref(dy.double(), xd.contiguous())
    del xd
    e = rel_err(dw, ref)
    print('f16x3 decode1 wgrad (4,512,1024): %.3g' % e)
    assert e < WGRAD_BIG_TOL, 'decode1 wgrad at (4,512,1024): %.3g' % e
    assert torch.equal(eng.segnet_train_wgrad_f16x3(dy, h, idx), dw)


@pytest.mark.parametrize('shape', [(2, 48, 80), (2, 6, 10)])
def test_dynamic_range(eng, shape):
    """inputs at 2^20, dy at 2^-30, weights at 2^-12: the per-tensor scales keep every plane inside f16's range"""
    e = [check_forward(eng, shape, 11, xs=X_SCALE, ws=W_SCALE),
         check_dgrad(eng, shape, 12, dys=DY_SCALE, ws=W_SCALE),
         check_wgrad(eng, shape, 13, xs=X_SCALE, dys=DY_SCALE)]
    print('f16x3 dynamic range %s: forward %.3g, dgrad %.3g, wgrad %.3g' % ((shape,) + tuple(e)))


def test_all_zero_operands_give_exact_zeros(eng):
    B, H, W = 2, 32, 64
    img, x, h, idx, dy, w1, w64 = inputs(B, H, W, 21)
    wt = torch.from_numpy(segnet.pack_weight(w64.numpy())).cuda()
    z = torch.zeros((B, H, W, 64), device='cuda')
    zh = torch.zeros((B, H // 2, W // 2, 64), device='cuda')
    y, stats = eng.segnet_train_forward_f16x3(z, wt)
    assert torch.equal(y, torch.zeros_like(y)) and torch.equal(stats, torch.zeros_like(stats))
    y, stats = eng.segnet_train_forward_f16x3(zh, wt, idx.cuda())
    assert torch.equal(y, torch.zeros_like(y)) and torch.equal(stats, torch.zeros_like(stats))
    y, _ = eng.segnet_train_forward_f16x3(x.cuda(), torch.zeros_like(wt))
    assert torch.equal(y, torch.zeros_like(y))
    for ii in (None, idx.cuda()):
        dx = eng.segnet_train_dgrad_f16x3(z, wt, ii)
        assert torch.equal(dx, torch.zeros_like(dx))
    for xin, ii in ((x.cuda(), None), (h.cuda(), idx.cuda())):
        dw = eng.segnet_train_wgrad_f16x3(z, xin, ii)
        assert torch.equal(dw, torch.zeros_like(dw))
    dw = eng.segnet_train_wgrad_f16x3(dy.cuda(), z)
    assert torch.equal(dw, torch.zeros_like(dw))
    dw = eng.segnet_train_wgrad_f16x3(z, img.cuda(), None, segnet.MEAN, segnet.STD)
    assert torch.equal(dw, torch.zeros_like(dw))


def test_refusals_match_float32_and_write_nothing(eng):
    lib, ctx = eng._lib, eng._ctx
    s = eng._s()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    x = torch.randn((1, 25, 32, 64), device='cuda')                  # H odd
    x16 = torch.randn((1, 16, 32, 64), device='cuda')
    wt = torch.randn((49, 64, 64), device='cuda')
    img = torch.randn((1, 3, 16, 24), device='cuda')                 # conv1: W not a multiple of 16
    wt_off = torch.randn((49 * 64 * 64 + 4,), device='cuda')[1:]     # weights not 16-byte aligned
    x_off = torch.randn((16 * 32 * 64 + 4,), device='cuda')[1:]
    out, buf = poisoned((1, 25, 32, 64))
    dw, dbuf = poisoned((49, 64, 64))
    m3 = (ctypes.c_float * 3)(1, 1, 1)
    fwd = lambda x_, idx, lay, B, H, W, C, w, m, sd: ('spa_segnet_train_forward', (ctx, p(x_), idx, lay, B, H, W, C,
                                                                                   p(w), m, sd, p(out), None, s))
    dgr = lambda dy, w, idx, B, H, W: ('spa_segnet_train_dgrad', (ctx, p(dy), p(w), idx, B, H, W, p(out), s))
    wgr = lambda dy, x_, idx, lay, B, H, W, C, m, sd: ('spa_segnet_train_wgrad', (ctx, p(dy), p(x_), idx, lay, B, H, W,
                                                                                  C, m, sd, p(dw), s))
    calls = [
        fwd(x, None, 0, 1, 25, 32, 64, wt, None, None),              # H odd
        dgr(x, wt, None, 1, 25, 32),
        wgr(x, x, None, 0, 1, 25, 32, 64, None, None),
        wgr(x16, x16, None, 1, 1, 16, 32, 64, None, None),           # planar 64-channel input
        fwd(img, None, 1, 1, 16, 24, 3, wt, m3, m3),                 # conv1 W % 16
        fwd(img, None, 0, 1, 16, 32, 3, wt, None, None),             # conv1 without mean / std, channels-last
        fwd(img, None, 0, 1, 16, 32, 3, wt, m3, m3),                 # conv1 channels-last
        dgr(x16, wt_off, None, 1, 16, 32),                           # weights not aligned
        fwd(x_off, None, 0, 1, 16, 32, 64, wt, None, None),          # input not aligned
        wgr(x_off, x16, None, 0, 1, 16, 32, 64, None, None),         # dy not aligned
        fwd(x16, None, 0, 0, 16, 32, 64, wt, None, None),            # B = 0
        fwd(x16, None, 0, 1, 16, 32, 5, wt, None, None),             # Cin 5
        dgr(x16, wt, ctypes.c_void_p(x16.data_ptr() + 2), 1, 16, 32),  # index map not 4-byte aligned
        ('spa_segnet_train_forward', (ctx, None, None, 0, 1, 16, 32, 64, p(wt), None, None, p(out), None, s)),
        ('spa_segnet_train_dgrad', (ctx, p(x16), p(wt), None, 1, 16, 32, None, s)),
        ('spa_segnet_train_wgrad', (ctx, p(x16), None, None, 0, 1, 16, 32, 64, None, None, p(dw), s)),
    ]
    for i, (name, a) in enumerate(calls):
        rc32 = getattr(lib, name)(*a)
        rc = getattr(lib, name + '_f16x3')(*a)
        assert rc32 != 0, 'case %d: the float32 %s takes it' % (i, name)
        assert rc == rc32, 'case %d: %s_f16x3 returned %d, the float32 entry point %d' % (i, name, rc, rc32)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all().item() and torch.isnan(dbuf).all().item()


def test_same_bits_across_contexts(eng):
    engine = importlib.import_module('superpixel-align_amd.engine')
    B, H, W = 2, 48, 80
    img, x, h, idx, dy, w1, w64 = inputs(B, H, W, 31)
    wt = torch.from_numpy(segnet.pack_weight(w64.numpy())).cuda()
    w1t = torch.from_numpy(segnet.pack_weight(w1.numpy())).cuda()
    x, h, idx, dy, img = x.cuda(), h.cuda(), idx.cuda(), dy.cuda(), img.cuda()

    def run(e):
        return [*e.segnet_train_forward_f16x3(img, w1t, None, segnet.MEAN, segnet.STD),
                *e.segnet_train_forward_f16x3(h, wt, idx), e.segnet_train_dgrad_f16x3(dy, wt, idx),
                e.segnet_train_wgrad_f16x3(dy, x), e.segnet_train_wgrad_f16x3(dy, img, None, segnet.MEAN, segnet.STD)]

    a = run(eng)
    e2 = engine.Engine()
    try:
        b = run(e2)
        torch.cuda.synchronize()
    finally:
        e2.close()
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), 'output %d differs between contexts' % i


# ------------------------------------------------------------------------------- one whole training step
# The float32 step's bounds (tests/test_gpu_segnet_train.py) against the float64 restatement with unrounded operands.
# Measured: loss 5.3e-8; updates within the float32 step's own errors (worst the BN gammas, 1.4e-3 in both; conv1/W
# 1.7e-4, conv1_bn/beta 4.2e-6, a near-zero cancellation residual that float32 gets 4.3e-6 on); running statistics
# worst 2.8e-6 (float32 3.9e-6).
STEP_TOL = 5e-3
STAT_TOL = 3e-5
LOSS_TOL = 1e-5


def test_full_split_plane_step_against_float64(eng):
    B, H, W = 2, 64, 128
    p = st.init_params(5)
    g = torch.Generator().manual_seed(6)
    img = torch.rand((B, 3, H, W), generator=g) * 255
    t = torch.randint(-1, 2, (B, H, W), generator=g)
    tr = st.SegNetTrainer(p, st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy, engine=eng,
                          split_planes=True)
    before = {k: v.clone() for k, v in tr.P.items()}
    trace = []
    loss = tr.step(img.cuda(), t.cuda(), trace)
    P64 = {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=True) for k in st.PARAM_KEYS}
    S64 = {k: torch.tensor(p[k], dtype=torch.float64) for k in st.STAT_KEYS}
    maps = [m.cpu() for m in trace]
    l64, _ = st.reference_loss(P64, S64, img.double(), t, st.softmax_cross_entropy, idx_maps=maps)
    grads = dict(zip(P64.keys(), torch.autograd.grad(l64, list(P64.values()))))
    with torch.no_grad():
        Q = {k: v.detach().clone() for k, v in P64.items()}
        st.MomentumSGD(0.01, weight_decay=0.0005).update(Q, grads)
    el = abs(loss - l64.item()) / abs(l64.item())
    worst = {}
    for k in st.PARAM_KEYS:
        d_gpu = (tr.P[k].double().cpu() - before[k].double().cpu())
        d_ref = Q[k] - P64[k].detach()
        worst[k] = float((d_gpu - d_ref).abs().max() / d_ref.abs().max())
    es = {k: float((tr.S[k].double().cpu() - S64[k]).abs().max() / S64[k].abs().max()) for k in st.STAT_KEYS}
    ku, ks = max(worst, key=worst.get), max(es, key=es.get)
    print('f16x3 step: loss error %.3g, worst update error %.3g (%s), worst running statistic error %.3g (%s)'
          % (el, worst[ku], ku, es[ks], ks))
    assert el < LOSS_TOL, 'loss %.9g vs float64 %.9g' % (loss, l64.item())
    assert worst[ku] < STEP_TOL, '%s: update error %.3g' % (ku, worst[ku])
    assert es[ks] < STAT_TOL, '%s: running statistic error %.3g' % (ks, es[ks])


def test_split_plane_step_repeats_bit_for_bit(eng):
    B, H, W = 2, 32, 64
    p = st.init_params(7)
    g = torch.Generator().manual_seed(8)
    img = (torch.rand((B, 3, H, W), generator=g) * 255).cuda()
    t = torch.randint(-1, 2, (B, H, W), generator=g).cuda()
    runs = []
    for _ in range(2):
        tr = st.SegNetTrainer(p, st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy, engine=eng,
                              split_planes=True)
        losses = [tr.step(img, t) for _ in range(2)]
        runs.append((losses, {k: v.clone() for k, v in tr.P.items()}))
    assert runs[0][0] == runs[1][0]
    for k in st.PARAM_KEYS:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


# ------------------------------------------------------------------------------- end to end
# The float32 end-to-end test's settings and bounds (tests/test_gpu_segnet_train.py).
E2E_ITERS = 40
E2E_LOSS_FRACTION = 0.35
E2E_MIN_IOU = 0.6


def _run(args, cwd):
    r = subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_train_split_planes_then_label_end_to_end(tmp_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import segnet_train_synth as syn
    z = syn.write(str(tmp_path / 'data'), 8, 3, 64, 128)
    common = ['--train_img_zip', z[0], '--train_label_zip', z[1], '--val_img_zip', z[2], '--val_label_zip', z[3],
              '--batchsize', '2', '--input_shape', '64', '128', '--eval_shape', '64', '128',
              '--train_limit', str(E2E_ITERS), 'iteration', '--val_interval', '20', 'iteration',
              '--log_interval', '10', 'iteration', '--decay_iteration', '30']
    d1, d2 = str(tmp_path / 'run'), str(tmp_path / 'resumed')
    script = os.path.join(ROOT, 'train_segnet.py')
    _run([script, '--split_planes'] + common + ['--result_dir', d1], ROOT)
    log = json.load(open(os.path.join(d1, 'log')))
    print('f16x3 end to end: loss %s, road IoU %.4f' % ([round(e['main/loss'], 4) for e in log],
                                                       log[-1]['val/main/iou/road']))
    assert [e['iteration'] for e in log] == [10, 20, 30, 40]
    assert log[-1]['main/loss'] < E2E_LOSS_FRACTION * log[0]['main/loss'], [e['main/loss'] for e in log]
    assert log[-1]['val/main/iou/road'] > E2E_MIN_IOU, log[-1]
    args = json.load(open(os.path.join(d1, 'args.txt')))
    assert args['split_planes'] is True and args['dtype'] == 'fp32' and args['model'] == 'basic'
    snap20 = os.path.join(d1, 'snapshot_iter_20')
    assert st.snapshot_split_planes(snap20) and st.snapshot_dtype(snap20) == 'fp32'
    # --resume from the middle with the same flag reaches the same snapshot, bit for bit
    _run([script, '--split_planes'] + common + ['--result_dir', d2, '--resume', snap20], ROOT)
    with np.load(os.path.join(d1, 'snapshot_iter_40')) as a, np.load(os.path.join(d2, 'snapshot_iter_40')) as b:
        assert set(a.files) == set(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), k
    # labels_from_segnet.py (save_labels) reads the split-plane snapshot and predicts what the validation predicted
    out = str(tmp_path / 'labels')
    _run([os.path.join(ROOT, 'labels_from_segnet.py'), '--param_dir', d1, '--iteration', str(E2E_ITERS),
          '--img_zip_fn', z[2], '--label_zip_fn', z[3], '--out_dir', out, '--start_index', '0', '--end_index', '3',
          '--eval_shape', '64', '128', '--no_figure'], ROOT)
    res = [json.loads(l) for l in open(os.path.join(out, 'result.json')) if l.strip()]
    FP = sum(r['FP'] for r in res)
    FN = sum(r['FN'] for r in res)
    TP = sum(r['TP'] for r in res)
    assert (FP, FN) == (log[-1]['val_/main/FP'], log[-1]['val_/main/FN'])
    assert TP / float(TP + FP + FN) == log[-1]['val/main/iou/road']
