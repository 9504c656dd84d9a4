"""The one float64 restatement of SegNet-Basic (models/segnet_basic.py: torch CPU ops and Chainer's LRN formula) and
the numeric helpers and shared test bodies of tests/test_gpu_segnet*.py and tests/test_segnet_cpu.py.

What used to differ between the per-file copies is an argument here, and every call site passes its own value:
  family    the Engine / C entry point suffix: '' (float32), '_bf16', '_f16x3'
  operand   how a float32 operand enters the float64 reference: d64 (as it is) or r16 (rounded to bf16 first)
  tolerances and caps: no bound has a default in this module; the test files keep their constants and pass them
  what / label: the text that leads a printed figure or an assertion message
The two pooling rules stay two functions (check_pool_near_ties / check_pool_decided, and near_tie_indices /
decided_indices for forward64): "indices equal outside near-ties" is the float32 and bf16 kernels' claim, "decided
windows, all-negative windows exactly 0, undecided share capped" the split-plane kernels'."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

F = torch.nn.functional
segnet = importlib.import_module('superpixel-align_amd.segnet')
st = importlib.import_module('superpixel-align_amd.segnet_train')


def random_params(seed):
    """Chainer-layout parameters scaled so activations stay O(1)."""
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


# ------------------------------------------------------------------------------- operands and layouts
def t64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def d64(t):
    """a float32 operand as it is, as float64"""
    return t.float().double()


def r16(t):
    """the bf16 operand of a float32 value, as float64"""
    return st.bf16_round(torch.as_tensor(t).float()).double()


def nchw64(t):
    """a device tensor of logical shape (B,C,H,W) -> float64 on the CPU"""
    return t.detach().cpu().double()


def nchw(a):
    """(B,H,W,C) -> a (B,C,H,W) view"""
    return a.permute(0, 3, 1, 2)


def channels_last(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------- float64 layers
def standardise(x):
    """the dataset's two float32 operations on the 0..255 image"""
    x = np.asarray(x, np.float32).copy()
    x -= segnet.MEAN[None, :, None, None]
    x /= segnet.STD[None, :, None, None]
    return x


def lrn_chainer(x):
    """Chainer's local_response_normalization(x, 5, 1, 1e-4 / 5, 0.75): alpha NOT divided by n (3 channels: all)."""
    s = (x * x).sum(1, keepdim=True)                 # n = 5 covers all three channels
    return x * (1.0 + 1e-4 / 5 * s) ** -0.75


def conv7(h, w, b=None):
    """float64 7x7 convolution, padding 3, in strips of 64 output rows (bounded im2col memory at 512 x 1024)"""
    H = h.shape[2]
    hp = F.pad(h, (0, 0, 3, 3))
    return torch.cat([F.conv2d(hp[:, :, y0:min(y0 + 64, H) + 6], w, b, padding=(0, 3)) for y0 in range(0, H, 64)], 2)


def conv_bias(h, w64, b64):
    return conv7(h, w64) + b64[None, :, None, None]


def bn_conv(p, name, h):
    """the layer as the model states it: convolution, then BatchNorm in test mode"""
    y = conv7(h, t64(p[name + '/W']))
    g, be, mu, var = (t64(p['%s_bn/%s' % (name, k)])[None, :, None, None] for k in segnet.BN_PARAMS)
    return g * (y - mu) / torch.sqrt(var + segnet.BN_EPS) + be


def folded_conv(p, name, h):
    """the same layer with BatchNorm folded into the weights in float64"""
    w, b = segnet.fold_bn(p, np.float64)[name]
    return conv7(h, t64(w), t64(b))


def windows(h):
    B, C, H, W = h.shape
    return h.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def pool_argmax(h):
    win = windows(h)
    idx = win.argmax(-1)          # ties -> first (torch CPU argmax returns the first maximal index)
    return win.gather(-1, idx[..., None])[..., 0], idx


def unpool(h, idx):
    B, C, h2, w2 = h.shape
    out = torch.zeros(B, C, h2, w2, 4, dtype=h.dtype)
    out.scatter_(-1, idx.long()[..., None], h[..., None])
    return out.reshape(B, C, h2, w2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * h2, 2 * w2)


def classify(p, h):
    z = F.conv2d(h, t64(p['conv_classifier/W']), t64(p['conv_classifier/b']))
    return torch.softmax(z, 1)


def folded(p, name, ws=1.0, bs=1.0, operand=t64):
    """the layer's folded float32 weight and bias, scaled by the powers of two ws / bs (exact) ->
    (device packed weight, device bias, float64 (64,Cin,7,7) weight operand, float64 bias)"""
    w, b = segnet.fold_bn(p)[name]
    w = (w * np.float32(ws)).astype(np.float32)
    b = (b * np.float32(bs)).astype(np.float32)
    return (torch.from_numpy(segnet.pack_weight(w)).cuda(), torch.from_numpy(b).cuda(), operand(w), t64(b))


def classifier(p, ws=1.0):
    """the classifier's weight scaled by ws -> (device weight, device bias, float64 weight, float64 bias)"""
    wc, bc = segnet.fold_bn(p)['conv_classifier']
    wc = np.ascontiguousarray(wc * np.float32(ws)).astype(np.float32)
    return torch.from_numpy(wc).cuda(), torch.from_numpy(bc).cuda(), t64(wc), t64(bc)


# ------------------------------------------------------------------------------- the two pooling rules
def near_ties(ref, tol):
    top2 = windows(ref).sort(-1, descending=True).values
    return (top2[..., 0] - top2[..., 1]) < tol


def check_pool_near_ties(pooled, idx, ref, layer_tol, what):
    """values within layer_tol max|ref| of the oracle's window maximum; indices equal except where the window's top two
    oracle values are closer than that.  -> the value error as a fraction of max|ref|"""
    scale = float(ref.abs().max())
    tol = layer_tol * scale
    yv, yi = pool_argmax(ref)
    err = float((nchw64(pooled) - yv).abs().max())
    assert err <= tol, '%s: pooled error %.3g > %.3g' % (what, err, tol)
    bad = (idx.cpu().long() != yi) & ~near_ties(ref, tol)
    assert int(bad.sum()) == 0, '%s: %d pooling indices differ outside near-ties' % (what, int(bad.sum()))
    return err / scale


def decided_windows(v, tol):
    """v the float64 pre-ReLU output.  A window is decided if all four v <= -tol (index 0, value exactly 0) or if its
    maximum is >= tol and leads the runner-up by >= tol (index = argmax).
    -> (all-negative mask, leader mask, argmax)"""
    win = windows(v)
    srt = win.sort(-1, descending=True).values
    neg = (win <= -tol).all(-1)
    lead = (srt[..., 0] >= tol) & (srt[..., 0] - srt[..., 1] >= tol)
    return neg, lead, win.argmax(-1)


def pool_err(pooled, v):
    ref = torch.relu(v)
    return float((nchw64(pooled) - windows(ref).max(-1).values).abs().max()) / float(ref.abs().max())


def check_pool_decided(pooled, idx, v, layer_tol, exempt_windows, what):
    """pooled within layer_tol max|relu(v)| of the window maximum of relu(v) everywhere; the index of every decided
    window as decided_windows says; the undecided share capped.  -> the value error as a fraction of max|relu(v)|"""
    ref = torch.relu(v)
    scale = float(ref.abs().max())
    tol = layer_tol * scale
    err = float((nchw64(pooled) - windows(ref).max(-1).values).abs().max())
    neg, lead, arg = decided_windows(v, tol)
    exempt = 1.0 - float((neg | lead).double().mean())
    print('%s: pooled error %.3g of max|ref|, undecided windows %.3g' % (what, err / scale, exempt))
    assert err <= tol, '%s: pooled error %.3g > %.3g' % (what, err, tol)
    assert exempt <= exempt_windows, '%s: %.3g of the windows are undecided' % (what, exempt)
    di = idx.cpu().long()
    assert int((di[neg] != 0).sum()) == 0, '%s: an all-negative window has a non-zero index' % what
    assert bool((pooled.cpu()[neg] == 0.0).all()), '%s: an all-negative window is not exactly 0' % what
    bad = int((di[lead] != arg[lead]).sum())
    assert bad == 0, '%s: %d decided pooling indices differ' % (what, bad)
    return err / scale


def near_tie_indices(name, v, y, d, tol):
    """forward64's rule for the float32 kernels: the device's indices d, required equal to the oracle's outside
    near-ties of y = relu(v) and taken where the top two are closer than tol"""
    i = windows(y).argmax(-1)
    near = near_ties(y, tol)
    assert int(((d != i) & ~near).sum()) == 0, name
    return torch.where(near, d, i)


def decided_indices(name, v, y, d, tol):
    """forward64's rule for the split-plane kernels: the device's indices d, required to be decided_windows' in every
    decided window and taken as they are in the others"""
    neg, lead, arg = decided_windows(v, tol)
    assert int((d[neg] != 0).sum()) == 0 and int((d[lead] != arg[lead]).sum()) == 0, name
    print('%s at full size: undecided windows %.3g' % (name, 1.0 - float((neg | lead).double().mean())))
    return d


def forward64(p, x, dev_idx=None, rule=None, tol=None, layer=bn_conv):
    """x (B,3,H,W) float64, standardised -> (float64 probabilities (B,2,H,W), decode1's output).  dev_idx: the device's
    pooling indices, checked and adopted by rule (near_tie_indices or decided_indices) with tol max|y| per layer: a
    near-tie either side may resolve differently, and an unpooled value in the other position of its block is an O(1)
    change.  layer: bn_conv or folded_conv."""
    h = lrn_chainer(x)
    idxs = []
    for li, name in enumerate(segnet.ENCODERS):
        v = layer(p, name, h)
        y = torch.relu(v)
        if dev_idx is None:
            h, i = pool_argmax(y)
        else:
            i = rule(name, v, y, dev_idx[li].cpu().long(), tol * float(y.abs().max()))
            h = windows(y).gather(-1, i[..., None])[..., 0]
        idxs.append(i)
        del v, y
    for name, i in zip(segnet.DECODERS, idxs[::-1]):
        h = layer(p, name, unpool(h, i))
    return classify(p, h), h


# ------------------------------------------------------------------------------- inference: shared test bodies
def _entry(lib, stem, family):
    return getattr(lib, stem + family)


def check_outputs_written(eng, family, form):
    """one of the four forms ('conv1', 'enc', 'dec', 'dec1') through the C entry point into NaN / 255 poisoned outputs
    with a guard past the end.  (48, 80) and (6, 10) do not fill the 8 x 32 tiles: ragged right and bottom edges"""
    lib, ctx = eng._lib, eng._ctx
    enc, dec = _entry(lib, 'spa_segnet_encode', family), _entry(lib, 'spa_segnet_decode', family)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    poison = lambda n, dtype, fill: torch.full((n + 4096,), fill, dtype=dtype, device='cuda')
    p = random_params(38)
    B, H, W = (2, 48, 80) if form in ('conv1', 'dec1') else (3, 6, 10)
    g = torch.Generator().manual_seed(39)
    NHWC, NCHW = 0, 1
    if form in ('conv1', 'enc'):
        n = B * (H // 2) * (W // 2) * 64
        out = poison(n, torch.float32, float('nan'))
        oi = poison(n, torch.uint8, 255)
        if form == 'conv1':
            x = (torch.rand((B, 3, H, W), generator=g) * 255).cuda()
            w, b, _, _ = folded(p, 'conv1')
            m = (ctypes.c_float * 3)(*segnet.MEAN)
            sd = (ctypes.c_float * 3)(*segnet.STD)
            rc = enc(ctx, P(x), NCHW, B, H, W, 3, P(w), P(b), m, sd, P(out), P(oi), s)
        else:
            x = torch.randn((B, H, W, 64), generator=g).cuda()
            w, b, _, _ = folded(p, 'conv2')
            rc = enc(ctx, P(x), NHWC, B, H, W, 64, P(w), P(b), None, None, P(out), P(oi), s)
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
        wc, bc = classifier(p)[:2] if form == 'dec1' else (None, None)
        n = B * 2 * H * W if form == 'dec1' else B * H * W * 64
        out = poison(n, torch.float32, float('nan'))
        rc = dec(ctx, P(h), P(idx), NHWC, B, Hh, Wh, P(w), P(b), P(wc), P(bc), P(out), s)
        torch.cuda.synchronize()
        assert rc == 0
        assert not torch.isnan(out[:n]).any().item(), 'an output was not stored'
        assert torch.isnan(out[n:]).all().item(), 'a kernel wrote past its output'


def check_inference_refusals(eng, family):
    """the seven refused encode / decode calls return the float32 entry points' codes, launch nothing (the NaN / 9
    poisoned outputs stay as they were), and the engine wrapper raises on the same shapes"""
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

    def table(enc, dec):
        return [
            # conv1 at H = 40 (not a multiple of 16)
            enc(ctx, P(x3), NCHW, 1, 40, 48, 3, P(w3), P(b), m, sd, P(pooled), P(idx), s),
            # a 64-channel stage at an odd width
            enc(ctx, P(x64), NHWC, 1, 32, 31, 64, P(w64), P(b), None, None, P(pooled), P(idx), s),
            # Cin 16
            enc(ctx, P(x64), NHWC, 1, 32, 32, 16, P(w64), P(b), None, None, P(pooled), P(idx), s),
            # 64 channels stored planar
            enc(ctx, P(x64), NCHW, 1, 32, 32, 64, P(w64), P(b), None, None, P(pooled), P(idx), s),
            # conv1 image stored channels-last
            enc(ctx, P(x3), NHWC, 1, 48, 48, 3, P(w3), P(b), m, sd, P(pooled), P(idx), s),
            # decoder input stored planar
            dec(ctx, P(x64), P(idx), NCHW, 1, 16, 16, P(w64), P(b), None, None, P(pooled), s),
            # decode1 output 2 x (20, 20) = (40, 40): not a multiple of 16
            dec(ctx, P(x64), P(idx), NHWC, 1, 20, 20, P(w64), P(b), P(b), P(b), P(pooled), s),
        ]

    got = table(_entry(lib, 'spa_segnet_encode', family), _entry(lib, 'spa_segnet_decode', family))
    want = table(lib.spa_segnet_encode, lib.spa_segnet_decode)
    torch.cuda.synchronize()
    assert want == [-1, -1, -1, -4, -4, -4, -1]
    assert got == want
    assert torch.isnan(pooled).all().item() and bool((idx == 9).all())         # nothing was written
    encode = getattr(eng, 'segnet_encode' + family)
    with pytest.raises(Exception, match='-4'):
        encode(torch.zeros((1, 64, 32, 32), device='cuda'), w64, b)
    with pytest.raises(Exception, match='-1'):
        encode(torch.zeros((1, 3, 40, 48), device='cuda'), w3, b, segnet.MEAN, segnet.STD)


def check_batch_position(model, imgs, layers=False):
    """the network's output for the second of three images has the same bits alone and in the batch, and the batch
    repeats bit for bit (layers: every layer's output and indices too)"""
    one = model.forward(imgs[1:2].contiguous())
    three = model.forward(imgs)
    again = model.forward(imgs)
    torch.cuda.synchronize()
    assert torch.equal(one[0], three[1])
    assert torch.equal(three, again)
    if layers:
        t1, t2 = [], []
        model.forward(imgs, trace=t1)
        model.forward(imgs, trace=t2)
        for (a, ai), (b, bi) in zip(t1, t2):
            assert torch.equal(a, b) and torch.equal(ai, bi)


# ------------------------------------------------------------------------------- training: helpers
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


def inputs(B, H, W, seed, xs=1.0, dys=1.0, ws=1.0):
    """the operands of every pass form, the maps scaled by xs, the output gradient by dys, the weights by ws"""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((B, 3, H, W), generator=g) * 255.0 * xs
    x = torch.randn((B, H, W, 64), generator=g) * xs
    h = torch.randn((B, H // 2, W // 2, 64), generator=g) * xs
    idx = torch.randint(0, 4, (B, H // 2, W // 2, 64), generator=g, dtype=torch.uint8)
    dy = torch.randn((B, H, W, 64), generator=g) * dys
    w1 = torch.randn((64, 3, 7, 7), generator=g) * (2.0 / 147) ** 0.5 * ws
    w64 = torch.randn((64, 64, 7, 7), generator=g) * (2.0 / 3136) ** 0.5 * ws
    return img, x, h, idx, dy, w1, w64


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


def conv1_operand(eng, img, check):
    """conv1's float32 input exactly as the float32 kernels load it (standardised, LRN in float32): the float32 forward
    pass with a centre-tap identity weight returns it (one exact product per output), (B,H,W,3) float32 on the CPU.
    check: also hold it to within 1e-5 of the float64 restatement st.conv1_input (images on the 0..255 scale only)"""
    wid = torch.zeros((64, 3, 7, 7))
    for c in range(3):
        wid[c, c, 3, 3] = 1.0
    wt = torch.from_numpy(segnet.pack_weight(wid.numpy())).cuda()
    img = torch.as_tensor(img)
    y, _ = eng.segnet_train_forward(img.cuda().contiguous(), wt, None, segnet.MEAN, segnet.STD, stats=False)
    x1 = y[..., :3].cpu()
    if check:
        assert (x1.double() - st.conv1_input(img.double()).permute(0, 2, 3, 1)).abs().max() < 1e-5
    return x1


def ref_forms(eng, img, x, h, idx, operand, device_conv1, check_conv1):
    """float64 (B,C,H,W) operands of the three input forms: conv1's image, the map, the unpooled map.  device_conv1:
    conv1's input is the device's own float32 operand (conv1_operand; None where H is no multiple of 16) through
    `operand`; otherwise the float64 restatement st.conv1_input"""
    if not device_conv1:
        x1 = st.conv1_input(img.double())
    else:
        x1 = nchw(operand(conv1_operand(eng, img, check_conv1))) if img.shape[2] % 16 == 0 else None
    return x1, nchw(operand(x)), st.unpool_ref(nchw(operand(h)), nchw(idx.long()))


def _tag(shape, scales):
    return '%s %s' % (shape, scales) if scales else '%s' % (shape,)


# ------------------------------------------------------------------------------- training: shared test bodies
def check_forward(eng, shape, seed, family, operand, device_conv1, check_conv1, fwd_tol, bn_tol, **scales):
    """the three forward forms (conv1 where H is a multiple of 16) into poisoned outputs: against the float64
    convolution of the operands, the BatchNorm partial sums against float64 sums of the kernel's own y, and a repeat
    with the same bits.  -> the worst forward error as a fraction of max|ref|"""
    B, H, W = shape
    forward = getattr(eng, 'segnet_train_forward' + family)
    img, x, h, idx, dy, w1, w64 = inputs(B, H, W, seed, **scales)
    x1, xe, xd = ref_forms(eng, img, x, h, idx, operand, device_conv1, check_conv1)
    cases = [('conv1', img, None, w1, x1), ('enc', x, None, w64, xe), ('dec', h, idx, w64, xd)]
    worst = 0.0
    for name, xin, ii, w, xref in cases[1:] if H % 16 else cases:
        wt = torch.from_numpy(segnet.pack_weight(w.numpy())).cuda()
        out, buf = poisoned((B, H, W, 64))
        ii = ii.cuda() if ii is not None else None
        y, stats = forward(xin.cuda().contiguous(), wt, ii, segnet.MEAN, segnet.STD, out=out)
        torch.cuda.synchronize()
        check_guard(buf, B * H * W * 64)
        assert not torch.isnan(y).any().item(), '%s: an output was not stored' % name
        ref = F.conv2d(xref, operand(w), padding=3)                  # (B,64,H,W)
        e = rel_err(nchw(y), ref)
        worst = max(worst, e)
        assert e < fwd_tol, '%s %s: forward error %.3g' % (name, _tag(shape, scales), e)
        y64 = y.double()
        s_ref = torch.stack([y64.sum((0, 1, 2)), (y64 * y64).sum((0, 1, 2))])
        scale = torch.stack([y64.abs().sum((0, 1, 2)), (y64 * y64).sum((0, 1, 2))])
        es = float(((stats - s_ref).abs() / scale).max())
        assert es < bn_tol, '%s %s: BN sum error %.3g' % (name, shape, es)
        y2, stats2 = forward(xin.cuda().contiguous(), wt, ii, segnet.MEAN, segnet.STD)
        assert torch.equal(y2, y) and torch.equal(stats2, stats), '%s: repeat differs' % name
    return worst


def check_dgrad(eng, shape, seed, family, operand, fwd_tol, **scales):
    """the encoder's full-resolution input gradient and the decoder's gradient at the pooled input (through the index
    map) against float64 autograd on the operands, into poisoned outputs, each repeated.  -> the worst error"""
    B, H, W = shape
    dgrad = getattr(eng, 'segnet_train_dgrad' + family)
    img, x, h, idx, dy, w1, w64 = inputs(B, H, W, seed, **scales)
    wt = torch.from_numpy(segnet.pack_weight(w64.numpy())).cuda()
    dyd = dy.cuda().contiguous()
    xe = nchw(operand(x)).requires_grad_(True)
    F.conv2d(xe, operand(w64), padding=3).backward(nchw(operand(dy)))
    out, buf = poisoned((B, H, W, 64))
    dx = dgrad(dyd, wt, out=out)
    torch.cuda.synchronize()
    check_guard(buf, B * H * W * 64)
    assert not torch.isnan(dx).any().item()
    e1 = rel_err(nchw(dx), xe.grad)
    assert e1 < fwd_tol, 'enc dgrad %s: %.3g' % (_tag(shape, scales), e1)
    assert torch.equal(dgrad(dyd, wt), dx)
    hd = nchw(operand(h)).requires_grad_(True)
    F.conv2d(st.unpool_ref(hd, nchw(idx.long())), operand(w64), padding=3).backward(nchw(operand(dy)))
    out, buf = poisoned((B, H // 2, W // 2, 64))
    dh = dgrad(dyd, wt, idx.cuda(), out=out)
    torch.cuda.synchronize()
    check_guard(buf, B * H * W * 16)
    assert not torch.isnan(dh).any().item()
    e2 = rel_err(nchw(dh), hd.grad)
    assert e2 < fwd_tol, 'dec dgrad %s: %.3g' % (_tag(shape, scales), e2)
    assert torch.equal(dgrad(dyd, wt, idx.cuda()), dh)
    return max(e1, e2)


def check_wgrad(eng, shape, seed, family, operand, device_conv1, check_conv1, wgrad_tol, **scales):
    """the three weight gradient forms (conv1 where H is a multiple of 16; its channel 3 exactly zero) against
    wgrad_ref on the operands, into poisoned outputs, each repeated.  -> the worst error"""
    B, H, W = shape
    wgrad = getattr(eng, 'segnet_train_wgrad' + family)
    img, x, h, idx, dy, w1, w64 = inputs(B, H, W, seed, **scales)
    x1, xe, xd = ref_forms(eng, img, x, h, idx, operand, device_conv1, check_conv1)
    dyd = dy.cuda().contiguous()
    dyr = operand(dy).cuda()
    cases = [('conv1', img, None, x1, 4), ('enc', x, None, xe, 64), ('dec', h, idx, xd, 64)]
    worst = 0.0
    for name, xin, ii, xref, cp in cases[1:] if H % 16 else cases:
        out, buf = poisoned((49, 64, cp))
        ii = ii.cuda() if ii is not None else None
        dw = wgrad(dyd, xin.cuda().contiguous(), ii, segnet.MEAN, segnet.STD, out=out)
        torch.cuda.synchronize()
        check_guard(buf, 49 * 64 * cp)
        assert not torch.isnan(dw).any().item(), '%s: an output was not stored' % name
        xr = F.pad(xref, (0, 0, 0, 0, 0, 1)) if cp == 4 else xref      # conv1: channel 3 is zero
        ref = wgrad_ref(dyr, xr.permute(0, 2, 3, 1).contiguous().cuda())
        e = rel_err(dw, ref)
        worst = max(worst, e)
        assert e < wgrad_tol, '%s wgrad %s: %.3g' % (name, _tag(shape, scales), e)
        if cp == 4:
            assert torch.equal(dw[:, :, 3], torch.zeros_like(dw[:, :, 3]))
        dw2 = wgrad(dyd, xin.cuda().contiguous(), ii, segnet.MEAN, segnet.STD)
        assert torch.equal(dw2, dw), '%s wgrad: repeat differs' % name
    return worst


def check_wgrad_decode1_full_size(eng, family, operand, big_tol, label=None):
    """decode1's weight gradient at B = 4, 512 x 1024: K = 2.1e6 products per output, split over the chunks"""
    B, H, W = 4, 512, 1024
    wgrad = getattr(eng, 'segnet_train_wgrad' + family)
    g = torch.Generator(device='cuda').manual_seed(4)
    h = torch.randn((B, H // 2, W // 2, 64), generator=g, device='cuda')
    idx = torch.randint(0, 4, (B, H // 2, W // 2, 64), generator=g, device='cuda', dtype=torch.uint8)
    dy = torch.randn((B, H, W, 64), generator=g, device='cuda')
    dw = wgrad(dy, h, idx)
    xd = st.unpool_ref(nchw(operand(h)), nchw(idx.long())).permute(0, 2, 3, 1)
    ref = wgrad_ref(operand(dy), xd.contiguous())
    del xd
    e = rel_err(dw, ref)
    if label:
        print('%s decode1 wgrad (4,512,1024): %.3g' % (label, e))
    assert e < big_tol, 'decode1 wgrad at (4,512,1024): %.3g' % e
    assert torch.equal(wgrad(dy, h, idx), dw)


def check_train_refusals(eng, family, unaligned_weights):
    """refused forward / dgrad / wgrad calls return non-zero and leave the poisoned outputs as they were"""
    lib, ctx = eng._lib, eng._ctx
    forward, dgrad, wgrad = (_entry(lib, 'spa_segnet_train_' + k, family) for k in ('forward', 'dgrad', 'wgrad'))
    s = eng._s()
    x = torch.randn((1, 25, 32, 64), device='cuda')                  # H odd
    wt = torch.randn((49, 64, 64), device='cuda')
    out, buf = poisoned((1, 25, 32, 64))
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    rc = forward(ctx, p(x), None, 0, 1, 25, 32, 64, p(wt), None, None, p(out), None, s)
    assert rc != 0
    rc = dgrad(ctx, p(x), p(wt), None, 1, 25, 32, p(out), s)
    assert rc != 0
    dw, dbuf = poisoned((49, 64, 64))
    rc = wgrad(ctx, p(x), p(x), None, 0, 1, 25, 32, 64, None, None, p(dw), s)
    assert rc != 0
    x16 = torch.randn((1, 16, 32, 64), device='cuda')
    rc = wgrad(ctx, p(x16), p(x16), None, 1, 1, 16, 32, 64, None, None, p(dw), s)   # planar 64
    assert rc != 0
    img = torch.randn((1, 3, 16, 24), device='cuda')                 # conv1: W not a multiple of 16
    m3 = (ctypes.c_float * 3)(1, 1, 1)
    rc = forward(ctx, p(img), None, 1, 1, 16, 24, 3, p(wt), m3, m3, p(out), None, s)
    assert rc != 0
    rc = forward(ctx, p(img), None, 0, 1, 16, 32, 3, p(wt), None, None, p(out), None, s)
    assert rc != 0                                                   # conv1 without mean / std, and channels-last
    if unaligned_weights:
        wt_off = torch.randn((49 * 64 * 64 + 4,), device='cuda')[1:]     # weights not 16-byte aligned
        rc = dgrad(ctx, p(x16), p(wt_off), None, 1, 16, 32, p(out), s)
        assert rc != 0
    torch.cuda.synchronize()
    assert torch.isnan(buf).all().item() and torch.isnan(dbuf).all().item()


def step_against_float64(eng, trainer_kw, bf16_operands=False):
    """one training step at B = 2, 64 x 128 (init_params(5), seed-6 batch) on the device and restated in float64 with
    the device's index maps.  -> dict: loss, l64, updates / stats (each key's error relative to the reference's
    max |update| / max |value|), maps, acts, and p, img, t for a second trainer"""
    B, H, W = 2, 64, 128
    p = st.init_params(5)
    g = torch.Generator().manual_seed(6)
    img = torch.rand((B, 3, H, W), generator=g) * 255
    t = torch.randint(-1, 2, (B, H, W), generator=g)
    tr = st.SegNetTrainer(p, st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy, engine=eng,
                          **trainer_kw)
    before = {k: v.clone() for k, v in tr.P.items()}
    trace = []
    loss = tr.step(img.cuda(), t.cuda(), trace)
    P64 = {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=True) for k in st.PARAM_KEYS}
    S64 = {k: torch.tensor(p[k], dtype=torch.float64) for k in st.STAT_KEYS}
    maps = [m.cpu() for m in trace]
    acts = []
    l64, _ = st.reference_loss(P64, S64, img.double(), t, st.softmax_cross_entropy, idx_maps=maps, acts=acts,
                               bf16_operands=bf16_operands)
    grads = dict(zip(P64.keys(), torch.autograd.grad(l64, list(P64.values()))))
    with torch.no_grad():
        Q = {k: v.detach().clone() for k, v in P64.items()}
        st.MomentumSGD(0.01, weight_decay=0.0005).update(Q, grads)
    updates = {}
    for k in st.PARAM_KEYS:
        d_gpu = (tr.P[k].double().cpu() - before[k].double().cpu())
        d_ref = Q[k] - P64[k].detach()
        updates[k] = float((d_gpu - d_ref).abs().max() / d_ref.abs().max())
    stats = {k: float((tr.S[k].double().cpu() - S64[k]).abs().max() / S64[k].abs().max()) for k in st.STAT_KEYS}
    return dict(loss=loss, l64=l64.item(), updates=updates, stats=stats, maps=maps, acts=acts, p=p, img=img, t=t)


def check_step_repeats(eng, **trainer_kw):
    """two trainers from the same parameters take two steps each: the same losses and the same parameter bits"""
    B, H, W = 2, 32, 64
    p = st.init_params(7)
    g = torch.Generator().manual_seed(8)
    img = (torch.rand((B, 3, H, W), generator=g) * 255).cuda()
    t = torch.randint(-1, 2, (B, H, W), generator=g).cuda()
    runs = []
    for _ in range(2):
        tr = st.SegNetTrainer(p, st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy, engine=eng,
                              **trainer_kw)
        losses = [tr.step(img, t) for _ in range(2)]
        runs.append((losses, {k: v.clone() for k, v in tr.P.items()}))
    assert runs[0][0] == runs[1][0]
    for k in st.PARAM_KEYS:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
