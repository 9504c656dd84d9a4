"""GPU tests of bf16 SegNet-Basic inference (spa_segnet_encode_bf16 / spa_segnet_decode_bf16, SegNetBasic(dtype='bf16'),
labels_from_segnet.py --dtype bf16): each of the four layer forms against a float64 restatement on the kernel's own
bf16 operands, full and bounded writes, determinism across batch positions, the refusals, the whole network at the
training size against a restatement that rounds every layer's operands to bf16, the fp32 default left as it was, and
the labelling driver end to end on a synthetic zipped dataset."""
import ctypes
import importlib
import json
import os
import shutil
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

# Layer bounds, as a fraction of max|ref|: the bf16 training forward test's.  The restatement multiplies the kernel's
# own bf16 operands in float64, so the products agree exactly and only the float32 accumulation order differs.
# Measured worst: 4.7e-7 on the small shapes, 1.0e-6 layer by layer at 2 x 512 x 1024; probabilities 1.8e-6.
LAYER_TOL = 1e-5
# decode1's probabilities, absolute (the float32 test's bound; the logits' error is the accumulation error above)
PROB_TOL = 1e-5


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


def random_params(seed):
    """Chainer-layout parameters scaled so activations stay O(1) (tests/test_gpu_segnet.py's)."""
    rng = np.random.default_rng(seed)
    p = {}
    for i, name in enumerate(segnet.LAYERS):
        cin = 3 if i == 0 else 64
        p[name + '/W'] = (rng.standard_normal((64, cin, 7, 7)) * np.sqrt(2.0 / (cin * 49))).astype(np.float32)
        p[name + '_bn/gamma'] = rng.uniform(0.5, 1.5, 64).astype(np.float32)
        p[name + '_bn/beta'] = rng.uniform(-0.2, 0.2, 64).astype(np.float32)
        p[name + '_bn/avg_mean'] = rng.uniform(-0.2, 0.2, 64).astype(np.float32)
        p[name + '_bn/avg_var'] = rng.uniform(0.5, 2.0, 64).astype(np.float32)
    p['conv_classifier/W'] = (rng.standard_normal((2, 64, 1, 1)) / 4).astype(np.float32)
    p['conv_classifier/b'] = rng.uniform(-0.1, 0.1, 2).astype(np.float32)
    return p


# ------------------------------------------------------------------------------- float64 restatement
def r16(t):
    """the bf16 operand of a float32 value, as float64"""
    return st.bf16_round(torch.as_tensor(t).float()).double()


def folded(p, name):
    """(device packed float32 weight, device bias, float64 (64,Cin,7,7) bf16 weight operand, float64 bias)"""
    w, b = segnet.fold_bn(p)[name]
    dev = (torch.from_numpy(segnet.pack_weight(w)).cuda(), torch.from_numpy(b).cuda())
    return dev + (r16(torch.from_numpy(w)), torch.from_numpy(b).double())


def conv7(h, w):
    """float64 7x7 convolution, padding 3, in strips of 64 output rows (bounded im2col memory at 512 x 1024)"""
    H = h.shape[2]
    hp = F.pad(h, (0, 0, 3, 3))
    return torch.cat([F.conv2d(hp[:, :, y0:min(y0 + 64, H) + 6], w, padding=(0, 3)) for y0 in range(0, H, 64)], 2)


def windows(h):
    B, C, H, W = h.shape
    return h.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def near_ties(ref, tol):
    top2 = windows(ref).sort(-1, descending=True).values
    return (top2[..., 0] - top2[..., 1]) < tol


def nchw64(t):
    """a (B,64,h,w) channels-last device tensor -> float64 CPU (B,64,h,w)"""
    return t.detach().cpu().double()


def conv1_operand(eng, img):
    """conv1's float32 input exactly as the kernels load it (standardised, LRN in float32): the float32 training
    forward with a centre-tap identity weight returns it (one exact product per output), (B,3,H,W) float32 on the CPU"""
    wid = torch.zeros((64, 3, 7, 7))
    for c in range(3):
        wid[c, c, 3, 3] = 1.0
    wt = torch.from_numpy(segnet.pack_weight(wid.numpy())).cuda()
    y, _ = eng.segnet_train_forward(torch.as_tensor(img).cuda().contiguous(), wt, None, segnet.MEAN, segnet.STD,
                                    stats=False)
    x1 = y[..., :3].permute(0, 3, 1, 2).cpu().contiguous()
    del y
    assert (x1.double() - st.conv1_input(torch.as_tensor(img).double())).abs().max() < 1e-5
    return x1


def check_pool(pooled, idx, ref, what):
    """values within LAYER_TOL max|ref| of the oracle's window maximum; indices equal except where the window's top two
    oracle values are closer than that (test_gpu_segnet.check_pool's rule)"""
    tol = LAYER_TOL * float(ref.abs().max())
    win = windows(ref)
    yi = win.argmax(-1)
    yv = win.gather(-1, yi[..., None])[..., 0]
    err = float((nchw64(pooled) - yv).abs().max())
    assert err <= tol, '%s: pooled error %.3g > %.3g' % (what, err, tol)
    bad = (idx.cpu().long() != yi) & ~near_ties(ref, tol)
    assert int(bad.sum()) == 0, '%s: %d pooling indices differ outside near-ties' % (what, int(bad.sum()))
    return err / float(ref.abs().max())


def channels_last(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------- the four forms
ENC_SHAPES = [(2, 48, 80), (3, 6, 10), (1, 16, 16)]        # (B, H, W) of the convolution: 6 x 10 is a 1/8 map of 48 x 80
CONV1_SHAPES = [(2, 48, 80), (1, 16, 32)]
DEC_SHAPES = [(2, 3, 5), (2, 24, 40), (1, 8, 16)]           # (B, Hh, Wh) of the pooled input
DEC1_SHAPES = [(2, 24, 40), (3, 8, 8)]                      # decode1: 2 Hh, 2 Wh multiples of 16


@pytest.mark.parametrize('shape', CONV1_SHAPES)
def test_conv1_against_float64(eng, shape):
    B, H, W = shape
    p = random_params(30)
    img = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(31)) * 255.0
    w, b, w64, b64 = folded(p, 'conv1')
    pooled, idx = eng.segnet_encode_bf16(img.cuda().contiguous(), w, b, segnet.MEAN, segnet.STD)
    torch.cuda.synchronize()
    assert pooled.shape == (B, 64, H // 2, W // 2) and pooled.is_contiguous(memory_format=torch.channels_last)
    ref = torch.relu(conv7(r16(conv1_operand(eng, img)), w64) + b64[None, :, None, None])
    e = check_pool(pooled, idx, ref, 'conv1 %s' % (shape,))
    print('conv1 %s: pooled error %.3g of max|ref|' % (shape, e))


@pytest.mark.parametrize('shape', ENC_SHAPES)
def test_encoder_64_against_float64(eng, shape):
    B, H, W = shape
    p = random_params(32)
    x = channels_last(torch.randn((B, 64, H, W), generator=torch.Generator().manual_seed(33)))
    w, b, w64, b64 = folded(p, 'conv3')
    pooled, idx = eng.segnet_encode_bf16(x, w, b)
    torch.cuda.synchronize()
    assert pooled.shape == (B, 64, H // 2, W // 2)
    ref = torch.relu(conv7(r16(x.cpu()), w64) + b64[None, :, None, None])
    e = check_pool(pooled, idx, ref, 'encoder %s' % (shape,))
    print('encoder %s: pooled error %.3g of max|ref|' % (shape, e))


def pooled_input(B, Hh, Wh, seed):
    """a pooled map and its index map as an encoder leaves them (non-negative values, every index 0..3)"""
    g = torch.Generator().manual_seed(seed)
    h = channels_last(torch.rand((B, 64, Hh, Wh), generator=g) * 2.0)
    idx = channels_last(torch.randint(0, 4, (B, 64, Hh, Wh), generator=g, dtype=torch.uint8))
    return h, idx


@pytest.mark.parametrize('shape', DEC_SHAPES)
def test_decoder_against_float64(eng, shape):
    B, Hh, Wh = shape
    p = random_params(34)
    h, idx = pooled_input(B, Hh, Wh, 35)
    w, b, w64, b64 = folded(p, 'conv_decode3')
    y = eng.segnet_decode_bf16(h, idx, w, b)
    torch.cuda.synchronize()
    assert y.shape == (B, 64, 2 * Hh, 2 * Wh) and y.is_contiguous(memory_format=torch.channels_last)
    ref = conv7(st.unpool_ref(r16(h.cpu()), idx.cpu().long()), w64) + b64[None, :, None, None]
    e = float((nchw64(y) - ref).abs().max()) / float(ref.abs().max())
    print('decoder %s: error %.3g of max|ref|' % (shape, e))
    assert e <= LAYER_TOL


@pytest.mark.parametrize('shape', DEC1_SHAPES)
def test_decode1_against_float64(eng, shape):
    B, Hh, Wh = shape
    p = random_params(36)
    h, idx = pooled_input(B, Hh, Wh, 37)
    w, b, w64, b64 = folded(p, 'conv_decode1')
    wc, bc = segnet.fold_bn(p)['conv_classifier']
    prob = eng.segnet_decode_bf16(h, idx, w, b, torch.from_numpy(wc).cuda(), torch.from_numpy(bc).cuda())
    torch.cuda.synchronize()
    assert prob.shape == (B, 2, 2 * Hh, 2 * Wh) and prob.is_contiguous()
    y = conv7(st.unpool_ref(r16(h.cpu()), idx.cpu().long()), w64) + b64[None, :, None, None]
    z = F.conv2d(y, torch.from_numpy(wc).double()[:, :, None, None], torch.from_numpy(bc).double())
    ref = torch.softmax(z, 1)
    e = float((prob.cpu().double() - ref).abs().max())
    print('decode1 %s: probability error %.3g' % (shape, e))
    assert e <= PROB_TOL


# ------------------------------------------------------------------------------- writes, through the C entry points
def _poisoned(n, dtype, fill, guard=4096):
    return torch.full((n + guard,), fill, dtype=dtype, device='cuda')


@pytest.mark.parametrize('form', ['conv1', 'enc', 'dec', 'dec1'])
def test_outputs_fully_written_and_bounded(eng, form):
    lib, ctx = eng._lib, eng._ctx
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    p = random_params(38)
    B, H, W = (2, 48, 80) if form in ('conv1', 'dec1') else (3, 6, 10)
    g = torch.Generator().manual_seed(39)
    NHWC, NCHW = 0, 1
    if form in ('conv1', 'enc'):
        n = B * (H // 2) * (W // 2) * 64
        out = _poisoned(n, torch.float32, float('nan'))
        oi = _poisoned(n, torch.uint8, 255)
        if form == 'conv1':
            x = (torch.rand((B, 3, H, W), generator=g) * 255).cuda()
            w, b, _, _ = folded(p, 'conv1')
            m = (ctypes.c_float * 3)(*segnet.MEAN)
            sd = (ctypes.c_float * 3)(*segnet.STD)
            rc = lib.spa_segnet_encode_bf16(ctx, P(x), NCHW, B, H, W, 3, P(w), P(b), m, sd, P(out), P(oi), s)
        else:
            x = torch.randn((B, H, W, 64), generator=g).cuda()
            w, b, _, _ = folded(p, 'conv2')
            rc = lib.spa_segnet_encode_bf16(ctx, P(x), NHWC, B, H, W, 64, P(w), P(b), None, None, P(out), P(oi), s)
        torch.cuda.synchronize()
        assert rc == 0
        assert not torch.isnan(out[:n]).any().item(), 'a pooled value was not stored'
        assert int(oi[:n].max()) <= 3, 'a pooling index was not stored'
        assert torch.isnan(out[n:]).all().item() and bool((oi[n:] == 255).all()), 'a kernel wrote past its output'
    else:
        Hh, Wh = H // 2, W // 2
        h = torch.rand((B, Hh, Wh, 64), generator=g).cuda()
        idx = torch.randint(0, 4, (B, Hh, Wh, 64), generator=g, dtype=torch.uint8).cuda()
        w, b, _, _ = folded(p, 'conv_decode1' if form == 'dec1' else 'conv_decode2')
        if form == 'dec1':
            wc, bc = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in segnet.fold_bn(p)['conv_classifier'])
            n = B * 2 * H * W
        else:
            wc = bc = None
            n = B * H * W * 64
        out = _poisoned(n, torch.float32, float('nan'))
        rc = lib.spa_segnet_decode_bf16(ctx, P(h), P(idx), NHWC, B, Hh, Wh, P(w), P(b),
                                        P(wc) if wc is not None else None, P(bc) if bc is not None else None,
                                        P(out), s)
        torch.cuda.synchronize()
        assert rc == 0
        assert not torch.isnan(out[:n]).any().item(), 'an output was not stored'
        assert torch.isnan(out[n:]).all().item(), 'a kernel wrote past its output'


# ------------------------------------------------------------------------------- determinism
def test_determinism_batch_position(eng):
    p = random_params(40)
    model = segnet.SegNetBasic(p, engine=eng, dtype='bf16')
    g = np.random.default_rng(41)
    imgs = torch.from_numpy(g.integers(0, 256, (3, 3, 48, 80)).astype(np.float32)).cuda()
    one = model.forward(imgs[1:2].contiguous())
    three = model.forward(imgs)
    again = model.forward(imgs)
    torch.cuda.synchronize()
    assert torch.equal(one[0], three[1])
    assert torch.equal(three, again)
    # every layer's output repeats bit for bit too
    t1, t2 = [], []
    model.forward(imgs, trace=t1)
    model.forward(imgs, trace=t2)
    for (a, ai), (b, bi) in zip(t1, t2):
        assert torch.equal(a, b) and torch.equal(ai, bi)


# ------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(eng):
    lib, ctx = eng._lib, eng._ctx
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    x3 = torch.zeros((1, 3, 48, 48), device='cuda')
    x64 = torch.zeros((1, 64, 32, 32), device='cuda')
    w3 = torch.zeros((49, 64, 4), device='cuda')
    w64 = torch.zeros((49, 64, 64), device='cuda')
    b = torch.zeros(64, device='cuda')
    pooled = torch.full((1 << 18,), float('nan'), device='cuda')
    idx = torch.full((1 << 18,), 9, dtype=torch.uint8, device='cuda')
    m = (ctypes.c_float * 3)(*segnet.MEAN)
    sd = (ctypes.c_float * 3)(*segnet.STD)
    NHWC, NCHW = 0, 1
    enc, dec = lib.spa_segnet_encode_bf16, lib.spa_segnet_decode_bf16
    cases = [
        # conv1 at H = 40 (not a multiple of 16)
        (enc(ctx, P(x3), NCHW, 1, 40, 48, 3, P(w3), P(b), m, sd, P(pooled), P(idx), s), -1),
        # a 64-channel stage at an odd width
        (enc(ctx, P(x64), NHWC, 1, 32, 31, 64, P(w64), P(b), None, None, P(pooled), P(idx), s), -1),
        # Cin 16
        (enc(ctx, P(x64), NHWC, 1, 32, 32, 16, P(w64), P(b), None, None, P(pooled), P(idx), s), -1),
        # 64 channels stored planar
        (enc(ctx, P(x64), NCHW, 1, 32, 32, 64, P(w64), P(b), None, None, P(pooled), P(idx), s), -4),
        # conv1 image stored channels-last
        (enc(ctx, P(x3), NHWC, 1, 48, 48, 3, P(w3), P(b), m, sd, P(pooled), P(idx), s), -4),
        # decoder input stored planar
        (dec(ctx, P(x64), P(idx), NCHW, 1, 16, 16, P(w64), P(b), None, None, P(pooled), s), -4),
        # decode1 output 2 x (20, 20) = (40, 40): not a multiple of 16
        (dec(ctx, P(x64), P(idx), NHWC, 1, 20, 20, P(w64), P(b), P(b), P(b), P(pooled), s), -1),
    ]
    # the float32 stages refuse the same calls with the same codes
    want = [
        lib.spa_segnet_encode(ctx, P(x3), NCHW, 1, 40, 48, 3, P(w3), P(b), m, sd, P(pooled), P(idx), s),
        lib.spa_segnet_encode(ctx, P(x64), NHWC, 1, 32, 31, 64, P(w64), P(b), None, None, P(pooled), P(idx), s),
        lib.spa_segnet_encode(ctx, P(x64), NHWC, 1, 32, 32, 16, P(w64), P(b), None, None, P(pooled), P(idx), s),
        lib.spa_segnet_encode(ctx, P(x64), NCHW, 1, 32, 32, 64, P(w64), P(b), None, None, P(pooled), P(idx), s),
        lib.spa_segnet_encode(ctx, P(x3), NHWC, 1, 48, 48, 3, P(w3), P(b), m, sd, P(pooled), P(idx), s),
        lib.spa_segnet_decode(ctx, P(x64), P(idx), NCHW, 1, 16, 16, P(w64), P(b), None, None, P(pooled), s),
        lib.spa_segnet_decode(ctx, P(x64), P(idx), NHWC, 1, 20, 20, P(w64), P(b), P(b), P(b), P(pooled), s),
    ]
    torch.cuda.synchronize()
    assert [rc for rc, _ in cases] == [w for _, w in cases]
    assert [rc for rc, _ in cases] == want
    assert torch.isnan(pooled).all().item() and bool((idx == 9).all())         # nothing was written
    with pytest.raises(Exception, match='-4'):
        eng.segnet_encode_bf16(torch.zeros((1, 64, 32, 32), device='cuda'), w64, b)
    with pytest.raises(Exception, match='-1'):
        eng.segnet_encode_bf16(torch.zeros((1, 3, 40, 48), device='cuda'), w3, b, segnet.MEAN, segnet.STD)


# ------------------------------------------------------------------------------- whole network
# conv1's float32 operand (standardisation + LRN, a powf per channel) is not bit-reproducible across compilation units:
# at 2 x 512 x 1024 the bf16 roundings of the float32 training kernel's operand and of the bf16 training kernel's
# differ at 24 of 3.1M values, and this kernel's differ from either at a similar rate.  Each such operand is one bf16
# step off, so the full-size conv1 check allows a small fraction of outputs beyond LAYER_TOL, with a bounded error.
# Measured (random_params(19), seed-20 image): 0.19 % of the 16.8M pooled values, worst 4.0e-4 of max|ref|.
CONV1_FLIP_FRACTION = 5e-3
CONV1_FLIP_TOL = 2e-3
# The free-running restatement starts from the device's conv1 output and then rounds each of its own float64 layer
# outputs to bf16: a value that the float32 accumulation moves across a bf16 rounding boundary becomes another operand
# (2^-8 relative), and with random weights these differences grow over the remaining seven layers until some pooling
# windows pick another position, an O(1) change there.  Measured worst at B = 2, 512 x 1024, predicted at
# 1024 x 2048: probability error 0.541, labels differing outside near-ties 1.12e-2 (the same layers checked one by one
# above stay within 1e-6).  Bounds with margin: they catch a network that is wrong, not the rounding's spread.
NET_PROB_TOL = 0.75
NET_NEAR = 2e-2                     # |p1 - p0| below this is a near-tie of the resized probabilities
NET_LABEL_FRACTION = 2.5e-2


def forward64_bf16(p, h1, dev_idx):
    """float64 SegNet-Basic from conv2 on, every layer's operands rounded to bf16: h1 the device's conv1 output
    (B,64,H/2,W/2); the device's pooling indices dev_idx (a near-tie may resolve either way).  -> (B,2,H,W)"""
    f = segnet.fold_bn(p)
    h, idxs = r16(h1.cpu()), [dev_idx[0].cpu().long()]
    for li, name in enumerate(segnet.ENCODERS[1:], 1):
        w, b = f[name]
        y = torch.relu(conv7(h, r16(torch.from_numpy(w))) + torch.from_numpy(b).double()[None, :, None, None])
        i = dev_idx[li].cpu().long()
        h = r16(windows(y).gather(-1, i[..., None])[..., 0])
        idxs.append(i)
    for name, i in zip(segnet.DECODERS, idxs[::-1]):
        w, b = f[name]
        h = conv7(st.unpool_ref(h, i), r16(torch.from_numpy(w))) + torch.from_numpy(b).double()[None, :, None, None]
        if name != 'conv_decode1':
            h = r16(h)
    wc, bc = f['conv_classifier']
    z = F.conv2d(h, torch.from_numpy(wc).double()[:, :, None, None], torch.from_numpy(bc).double())
    return torch.softmax(z, 1)


def test_predict_full_size(eng):
    p = random_params(19)
    g = np.random.default_rng(20)
    img = g.integers(0, 256, (2, 3, 512, 1024)).astype(np.float32)
    model = segnet.SegNetBasic(p, pred_shape=(1024, 2048), engine=eng, dtype='bf16')
    out = model.predict(img, return_score=True)
    trace = []
    prob = model.forward(torch.from_numpy(img).cuda(), trace=trace)   # the same launches: the indices predict used
    # 1. every layer at full size against float64 on the bf16 operands of the device's own input to it
    f = segnet.fold_bn(p)
    _, _, w64, b64 = folded(p, 'conv1')
    ref = torch.relu(conv7(r16(conv1_operand(eng, torch.from_numpy(img))), w64) + b64[None, :, None, None])
    err = (nchw64(trace[0][0]) - windows(ref).max(-1).values).abs() / float(ref.abs().max())
    flips = float((err > LAYER_TOL).double().mean())
    print('conv1 at full size: %.3g of the outputs beyond LAYER_TOL, worst %.3g of max|ref|' % (flips, float(err.max())))
    assert flips <= CONV1_FLIP_FRACTION and float(err.max()) <= CONV1_FLIP_TOL
    del ref, err
    worst = 0.0
    for name, (pooled, idx), (h, _) in zip(segnet.ENCODERS[1:], trace[1:], trace):
        _, _, w64, b64 = folded(p, name)
        ref = torch.relu(conv7(r16(h.cpu()), w64) + b64[None, :, None, None])
        worst = max(worst, check_pool(pooled, idx, ref, name))
    hd = trace[-1][0]
    for name, (_, idx) in zip(segnet.DECODERS, trace[::-1]):
        w, b, w64, b64 = folded(p, name)
        ref = conv7(st.unpool_ref(r16(hd.cpu()), idx.cpu().long()), w64) + b64[None, :, None, None]
        if name == 'conv_decode1':
            wc, bc = f['conv_classifier']
            hd = eng.segnet_decode_bf16(hd, idx, w, b, torch.from_numpy(wc).cuda(), torch.from_numpy(bc).cuda())
            z = F.conv2d(ref, torch.from_numpy(wc).double()[:, :, None, None], torch.from_numpy(bc).double())
            e1 = float((hd.cpu().double() - torch.softmax(z, 1)).abs().max())
            assert e1 <= PROB_TOL, 'decode1: probability error %.3g' % e1
        else:
            hd = eng.segnet_decode_bf16(hd, idx, w, b)
            e = float((nchw64(hd) - ref).abs().max()) / float(ref.abs().max())
            assert e <= LAYER_TOL, '%s: error %.3g of max|ref|' % (name, e)
            worst = max(worst, e)
    assert torch.equal(hd, prob)                                       # the layers above are the network's
    print('conv2 .. decode2 at full size: worst error %.3g of max|ref|, decode1 probabilities %.3g' % (worst, e1))
    # 2. the free-running restatement from the device's conv1 output (bounds: see NET_PROB_TOL)
    ref = forward64_bf16(p, trace[0][0], [i for _, i in trace]).numpy()
    worst_p, worst_l = 0.0, 0.0
    for bi in range(2):
        label, score = out[bi]
        assert label.shape == (1024, 2048) and score.shape == (2, 1024, 2048) and score.dtype == np.float32
        want = segnet.resize_bilinear_pil(ref[bi].astype(np.float32), (1024, 2048))
        worst_p = max(worst_p, float(np.abs(score - want).max()))
        near = np.abs(want[1] - want[0]) < NET_NEAR
        worst_l = max(worst_l, float((label[~near] != np.argmax(want, 0)[~near]).mean()))
    print('bf16 network, free-running restatement: probability error %.3g, labels differing outside near-ties %.3g'
          % (worst_p, worst_l))
    assert worst_p <= NET_PROB_TOL
    assert worst_l <= NET_LABEL_FRACTION


def test_fp32_dtype_is_a_no_op(eng):
    p = random_params(42)
    g = np.random.default_rng(43)
    x = torch.from_numpy(g.integers(0, 256, (2, 3, 64, 128)).astype(np.float32)).cuda()
    a = segnet.SegNetBasic(p, engine=eng).forward(x)
    b = segnet.SegNetBasic(p, engine=eng, dtype='fp32').forward(x)
    c = segnet.SegNetBasic(p, engine=eng, dtype='bf16').forward(x)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert not torch.equal(a, c)                                       # the bf16 network is another computation


# ------------------------------------------------------------------------------- labels_from_segnet.py end to end
# The float32 end-to-end test's settings and bounds (tests/test_gpu_segnet_train.py).
E2E_ITERS = 40
E2E_MIN_IOU = 0.6
# bf16 masks against the float32 masks of the same snapshot: the fraction of pixels that agree.  Measured: 1.0 minus
# 2e-4 at worst over the three 64 x 128 validation images; bound with margin.
E2E_MIN_AGREEMENT = 0.99
REF_KEYS = ['img_fn', 'label_fn', 'road_iou', 'non_road_iou', 'precision', 'recall', 'TP', 'FP', 'FN', 'param_dir',
            'iteration', 'gpu', 'img_zip_fn', 'label_zip_fn', 'out_dir', 'start_index', 'end_index', 'soft_label',
            'eval_shape', 'save_each', 'train_args']


def _run(args, cwd):
    r = subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _files(d):
    out = {}
    for fn in sorted(os.listdir(d)):
        with open(os.path.join(d, fn), 'rb') as f:
            out[fn] = f.read()
    return out


def test_train_then_label_bf16_end_to_end(tmp_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import segnet_train_synth as syn
    z = syn.write(str(tmp_path / 'data'), 8, 3, 64, 128)
    common = ['--train_img_zip', z[0], '--train_label_zip', z[1], '--val_img_zip', z[2], '--val_label_zip', z[3],
              '--batchsize', '2', '--input_shape', '64', '128', '--eval_shape', '64', '128',
              '--train_limit', str(E2E_ITERS), 'iteration', '--val_interval', '20', 'iteration',
              '--log_interval', '10', 'iteration', '--decay_iteration', '30']
    d1 = str(tmp_path / 'run')
    _run([os.path.join(ROOT, 'train_segnet.py')] + common + ['--result_dir', d1], ROOT)
    label_cmd = [os.path.join(ROOT, 'labels_from_segnet.py'), '--param_dir', d1, '--iteration', str(E2E_ITERS),
                 '--img_zip_fn', z[2], '--label_zip_fn', z[3], '--start_index', '0', '--end_index', '3',
                 '--eval_shape', '64', '128', '--no_figure']
    out_b, out_f = str(tmp_path / 'labels_bf16'), str(tmp_path / 'labels')
    _run(label_cmd + ['--out_dir', out_b, '--dtype', 'bf16'], ROOT)
    _run(label_cmd + ['--out_dir', out_f], ROOT)
    lines = [json.loads(l) for l in open(os.path.join(out_b, 'result.json')) if l.strip()]
    assert len(lines) == 3
    TP = FP = FN = 0
    agree, total = 0, 0
    for line in lines:
        assert list(line) == REF_KEYS + ['dtype'] and line['dtype'] == 'bf16'
        assert line['save_each'] is True and line['eval_shape'] == [64, 128]
        base = os.path.splitext(os.path.basename(line['img_fn']))[0]
        mask = np.load(os.path.join(out_b, base + '.npy'))
        assert mask.dtype == np.bool_ and mask.shape == (64, 128)
        assert np.array_equal(np.load(os.path.join(out_b, base + '_scores.npy')), mask)
        m32 = np.load(os.path.join(out_f, base + '.npy'))
        agree += int((mask == m32).sum())
        total += mask.size
        TP, FP, FN = TP + line['TP'], FP + line['FP'], FN + line['FN']
    iou = TP / float(TP + FP + FN)
    print('bf16 labels: road IoU %.4f, agreement with the float32 masks %.6f' % (iou, agree / float(total)))
    assert iou > E2E_MIN_IOU
    assert agree / float(total) >= E2E_MIN_AGREEMENT
    for line in (json.loads(l) for l in open(os.path.join(out_f, 'result.json')) if l.strip()):
        assert list(line) == REF_KEYS                                  # float32 lines: the reference's keys only
    # save_labels(save_each=False, dtype='bf16') returns the float32 scores at eval_shape
    sys.path.insert(0, ROOT)
    lfs = importlib.import_module('labels_from_segnet')
    res = lfs.save_labels(d1, E2E_ITERS, 0, z[2], z[3], str(tmp_path / 'mem'), 1, 2, False, [64, 128],
                          save_each=False, figure=False, dtype='bf16')
    assert len(res) == 2
    for k, v in res.items():
        if k.endswith('_scores'):
            assert v.dtype == np.float32 and v.shape == (2, 64, 128)
            assert np.array_equal(res[k[:-len('_scores')]], np.argmax(v, 0).astype(bool))
    # the float32 run with an explicit --dtype fp32 writes the same bytes as without it
    shutil.move(out_f, out_f + '_default')
    _run(label_cmd + ['--out_dir', out_f, '--dtype', 'fp32'], ROOT)
    assert _files(out_f) == _files(out_f + '_default')
