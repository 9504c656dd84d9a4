"""GPU tests of the SegNet-Basic training kernels (csrc/spa_segnet_train.hip, segnet_train.py): every forward, input
gradient and weight gradient form against float64 torch convolutions and their autograd, the BatchNorm partial sums,
NaN-poisoned outputs with a guard past the end, bit-identical repeats, refusals that write nothing, one whole training
step against the float64 restatement, and train_segnet.py -> labels_from_segnet.py end to end on synthetic zips."""
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

# Bounds, as a fraction of max|ref|.  Measured worst over the first three SHAPES: forward 2.4e-6 (conv1's float32 LRN
# load), dgrad 2.7e-6, wgrad 2.9e-7; decode1's wgrad at (4,512,1024) 1.4e-6.  Forward and dgrad forms keep the
# inference tests' 1e-5; wgrad sums up to K = B*H*W products per output (float32 within a chunk, float64 across the
# chunks), so it gets 1e-5 at the small shapes and 2e-5 at decode1's K = 2.1e6.
FWD_TOL = 1e-5
WGRAD_TOL = 1e-5
WGRAD_BIG_TOL = 2e-5


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


def inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((B, 3, H, W), generator=g) * 255.0
    x = torch.randn((B, H, W, 64), generator=g)
    h = torch.randn((B, H // 2, W // 2, 64), generator=g)
    idx = torch.randint(0, 4, (B, H // 2, W // 2, 64), generator=g, dtype=torch.uint8)
    dy = torch.randn((B, H, W, 64), generator=g)
    w1 = torch.randn((64, 3, 7, 7), generator=g) * (2.0 / 147) ** 0.5
    w64 = torch.randn((64, 64, 7, 7), generator=g) * (2.0 / 3136) ** 0.5
    return img, x, h, idx, dy, w1, w64


def nchw64(a):
    return a.double().permute(0, 3, 1, 2)


def ref_forms(img, x, h, idx):
    """float64 (B,C,H,W) inputs of the three forms: conv1's standardised LRN image, the map, the unpooled map"""
    x1 = st.conv1_input(img.double())
    return x1, nchw64(x), st.unpool_ref(nchw64(h), nchw64(idx.long()))


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_forms_and_bn_sums(eng, shape):
    B, H, W = shape
    img, x, h, idx, dy, w1, w64 = inputs(B, H, W, 1)
    x1, xe, xd = ref_forms(img, x, h, idx)
    cases = [('conv1', img, None, w1, x1), ('enc', x, None, w64, xe), ('dec', h, idx, w64, xd)]
    for name, xin, ii, w, xref in cases[1:] if H % 16 else cases:
        wt = torch.from_numpy(segnet.pack_weight(w.numpy())).cuda()
        out, buf = poisoned((B, H, W, 64))
        y, stats = eng.segnet_train_forward(xin.cuda().contiguous(), wt, ii.cuda() if ii is not None else None,
                                            segnet.MEAN, segnet.STD, out=out)
        torch.cuda.synchronize()
        check_guard(buf, B * H * W * 64)
        assert not torch.isnan(y).any().item(), '%s: an output was not stored' % name
        ref = F.conv2d(xref, w.double(), padding=3)                   # (B,64,H,W)
        e = rel_err(y.permute(0, 3, 1, 2), ref)
        assert e < FWD_TOL, '%s %s: forward error %.3g' % (name, shape, e)
        # the BN partial sums are the kernel's own y summed; compare with float64 sums of that y
        y64 = y.double()
        s_ref = torch.stack([y64.sum((0, 1, 2)), (y64 * y64).sum((0, 1, 2))])
        scale = torch.stack([y64.abs().sum((0, 1, 2)), (y64 * y64).sum((0, 1, 2))])
        es = float(((stats - s_ref).abs() / scale).max())
        assert es < 1e-6, '%s %s: BN sum error %.3g' % (name, shape, es)
        # repeat: the same bits
        y2, stats2 = eng.segnet_train_forward(xin.cuda().contiguous(), wt, ii.cuda() if ii is not None else None,
                                              segnet.MEAN, segnet.STD)
        assert torch.equal(y2, y) and torch.equal(stats2, stats), '%s: repeat differs' % name


@pytest.mark.parametrize('shape', SHAPES)
def test_dgrad_forms(eng, shape):
    B, H, W = shape
    img, x, h, idx, dy, w1, w64 = inputs(B, H, W, 2)
    wt = torch.from_numpy(segnet.pack_weight(w64.numpy())).cuda()
    dyd = dy.cuda().contiguous()
    # encoder: full-resolution input gradient
    xe = nchw64(x).requires_grad_(True)
    F.conv2d(xe, w64.double(), padding=3).backward(nchw64(dy))
    out, buf = poisoned((B, H, W, 64))
    dx = eng.segnet_train_dgrad(dyd, wt, out=out)
    torch.cuda.synchronize()
    check_guard(buf, B * H * W * 64)
    assert not torch.isnan(dx).any().item()
    e = rel_err(dx.permute(0, 3, 1, 2), xe.grad)
    assert e < FWD_TOL, 'enc dgrad %s: %.3g' % (shape, e)
    assert torch.equal(eng.segnet_train_dgrad(dyd, wt), dx)
    # decoder: the gradient at the pooled input, through the index map
    hd = nchw64(h).requires_grad_(True)
    F.conv2d(st.unpool_ref(hd, nchw64(idx.long())), w64.double(), padding=3).backward(nchw64(dy))
    out, buf = poisoned((B, H // 2, W // 2, 64))
    dh = eng.segnet_train_dgrad(dyd, wt, idx.cuda(), out=out)
    torch.cuda.synchronize()
    check_guard(buf, B * H * W * 16)
    assert not torch.isnan(dh).any().item()
    e = rel_err(dh.permute(0, 3, 1, 2), hd.grad)
    assert e < FWD_TOL, 'dec dgrad %s: %.3g' % (shape, e)
    assert torch.equal(eng.segnet_train_dgrad(dyd, wt, idx.cuda()), dh)


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


@pytest.mark.parametrize('shape', SHAPES)
def test_wgrad_forms(eng, shape):
    B, H, W = shape
    img, x, h, idx, dy, w1, w64 = inputs(B, H, W, 3)
    x1, xe, xd = ref_forms(img, x, h, idx)
    dyd = dy.cuda().contiguous()
    cases = [('conv1', img, None, x1, 4), ('enc', x, None, xe, 64), ('dec', h, idx, xd, 64)]
    for name, xin, ii, xref, cp in cases[1:] if H % 16 else cases:
        out, buf = poisoned((49, 64, cp))
        dw = eng.segnet_train_wgrad(dyd, xin.cuda().contiguous(), ii.cuda() if ii is not None else None,
                                    segnet.MEAN, segnet.STD, out=out)
        torch.cuda.synchronize()
        check_guard(buf, 49 * 64 * cp)
        assert not torch.isnan(dw).any().item(), '%s: an output was not stored' % name
        xr = F.pad(xref, (0, 0, 0, 0, 0, 1)) if cp == 4 else xref      # conv1: channel 3 is zero
        ref = wgrad_ref(dyd.double(), xr.permute(0, 2, 3, 1).contiguous().cuda())
        e = rel_err(dw, ref)
        assert e < WGRAD_TOL, '%s wgrad %s: %.3g' % (name, shape, e)
        if cp == 4:
            assert torch.equal(dw[:, :, 3], torch.zeros_like(dw[:, :, 3]))
        dw2 = eng.segnet_train_wgrad(dyd, xin.cuda().contiguous(), ii.cuda() if ii is not None else None,
                                     segnet.MEAN, segnet.STD)
        assert torch.equal(dw2, dw), '%s wgrad: repeat differs' % name


def test_wgrad_decode1_full_size(eng):
    """decode1's weight gradient at B = 4, 512 x 1024: K = 2.1e6 products per output, split over the chunks"""
    B, H, W = 4, 512, 1024
    g = torch.Generator(device='cuda').manual_seed(4)
    h = torch.randn((B, H // 2, W // 2, 64), generator=g, device='cuda')
    idx = torch.randint(0, 4, (B, H // 2, W // 2, 64), generator=g, device='cuda', dtype=torch.uint8)
    dy = torch.randn((B, H, W, 64), generator=g, device='cuda')
    dw = eng.segnet_train_wgrad(dy, h, idx)
    xd = st.unpool_ref(h.double().permute(0, 3, 1, 2), idx.long().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    ref = wgrad_ref(dy.double(), xd.contiguous())
    del xd
    e = rel_err(dw, ref)
    assert e < WGRAD_BIG_TOL, 'decode1 wgrad at (4,512,1024): %.3g' % e
    assert torch.equal(eng.segnet_train_wgrad(dy, h, idx), dw)


def test_refusals_write_nothing(eng):
    lib, ctx = eng._lib, eng._ctx
    s = eng._s()
    x = torch.randn((1, 25, 32, 64), device='cuda')                  # H odd
    wt = torch.randn((49, 64, 64), device='cuda')
    out, buf = poisoned((1, 25, 32, 64))
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    rc = lib.spa_segnet_train_forward(ctx, p(x), None, 0, 1, 25, 32, 64, p(wt), None, None, p(out), None, s)
    assert rc == -1 or rc != 0
    rc = lib.spa_segnet_train_dgrad(ctx, p(x), p(wt), None, 1, 25, 32, p(out), s)
    assert rc != 0
    dw, dbuf = poisoned((49, 64, 64))
    rc = lib.spa_segnet_train_wgrad(ctx, p(x), p(x), None, 0, 1, 25, 32, 64, None, None, p(dw), s)
    assert rc != 0
    x16 = torch.randn((1, 16, 32, 64), device='cuda')
    rc = lib.spa_segnet_train_wgrad(ctx, p(x16), p(x16), None, 1, 1, 16, 32, 64, None, None, p(dw), s)   # planar 64
    assert rc != 0
    img = torch.randn((1, 3, 16, 24), device='cuda')                 # conv1: W not a multiple of 16
    m3 = (ctypes.c_float * 3)(1, 1, 1)
    rc = lib.spa_segnet_train_forward(ctx, p(img), None, 1, 1, 16, 24, 3, p(wt), m3, m3, p(out), None, s)
    assert rc != 0
    rc = lib.spa_segnet_train_forward(ctx, p(img), None, 0, 1, 16, 32, 3, p(wt), None, None, p(out), None, s)
    assert rc != 0                                                   # conv1 without mean / std, and channels-last
    torch.cuda.synchronize()
    assert torch.isnan(buf).all().item() and torch.isnan(dbuf).all().item()


# ------------------------------------------------------------------------------- one whole training step
# every parameter's update, relative to its max |update|: measured worst 1.4e-3, on the BN gammas (their gradient
# sum(g * xhat) cancels heavily in float32); the convolution weights are far tighter
STEP_TOL = 5e-3
STAT_TOL = 3e-5          # running statistics, relative to max |value|; measured worst 3.9e-6


def test_full_training_step_against_float64(eng):
    B, H, W = 2, 64, 128
    p = st.init_params(5)
    g = torch.Generator().manual_seed(6)
    img = torch.rand((B, 3, H, W), generator=g) * 255
    t = torch.randint(-1, 2, (B, H, W), generator=g)
    tr = st.SegNetTrainer(p, st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy, engine=eng)
    before = {k: v.clone() for k, v in tr.P.items()}
    trace = []
    loss = tr.step(img.cuda(), t.cuda(), trace)
    P64 = {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=True) for k in st.PARAM_KEYS}
    S64 = {k: torch.tensor(p[k], dtype=torch.float64) for k in st.STAT_KEYS}
    maps = [m.cpu() for m in trace]
    acts = []
    l64, _ = st.reference_loss(P64, S64, img.double(), t, st.softmax_cross_entropy, idx_maps=maps, acts=acts)
    grads = dict(zip(P64.keys(), torch.autograd.grad(l64, list(P64.values()))))
    with torch.no_grad():
        Q = {k: v.detach().clone() for k, v in P64.items()}
        st.MomentumSGD(0.01, weight_decay=0.0005).update(Q, grads)
    assert abs(loss - l64.item()) < 1e-5 * abs(l64.item())
    for k in st.PARAM_KEYS:
        d_gpu = (tr.P[k].double().cpu() - before[k].double().cpu())
        d_ref = Q[k] - P64[k].detach()
        e = float((d_gpu - d_ref).abs().max() / d_ref.abs().max())
        assert e < STEP_TOL, '%s: update error %.3g' % (k, e)
    for k in st.STAT_KEYS:
        e = float((tr.S[k].double().cpu() - S64[k]).abs().max() / S64[k].abs().max())
        assert e < STAT_TOL, '%s: running statistic error %.3g' % (k, e)
    # the kernels' index maps are the first maximum wherever the float64 window is not a near-tie
    for m, a in zip(maps, acts):
        Bq, Hq, Wq, C = a.shape
        win = a.detach().reshape(Bq, Hq // 2, 2, Wq // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(Bq, Hq // 2, Wq // 2,
                                                                                                 C, 4)
        top2 = win.topk(2, -1).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-4 * float(a.abs().max())
        first = torch.argmax(win, -1)
        assert torch.equal(first[clear], m.long()[clear])
        assert float(clear.double().mean()) > 0.5


# ------------------------------------------------------------------------------- end to end
# Chosen from the float64 restatement of this task run on the CPU (same data, 40 iterations of MomentumSGD): the loss
# fell from 1.09 to 0.078 (first 10-iteration mean 0.6, last 0.07), and the validation road IoU was 0.65 after 10
# iterations and 0.785 after 40.
E2E_ITERS = 40
E2E_LOSS_FRACTION = 0.35
E2E_MIN_IOU = 0.6


def _run(args, cwd):
    r = subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_train_then_label_end_to_end(tmp_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import segnet_train_synth as syn
    z = syn.write(str(tmp_path / 'data'), 8, 3, 64, 128)
    common = ['--train_img_zip', z[0], '--train_label_zip', z[1], '--val_img_zip', z[2], '--val_label_zip', z[3],
              '--batchsize', '2', '--input_shape', '64', '128', '--eval_shape', '64', '128',
              '--train_limit', str(E2E_ITERS), 'iteration', '--val_interval', '20', 'iteration',
              '--log_interval', '10', 'iteration', '--decay_iteration', '30']
    d1, d2 = str(tmp_path / 'run'), str(tmp_path / 'resumed')
    _run([os.path.join(ROOT, 'train_segnet.py')] + common + ['--result_dir', d1], ROOT)
    log = json.load(open(os.path.join(d1, 'log')))
    assert [e['iteration'] for e in log] == [10, 20, 30, 40]
    assert log[-1]['main/loss'] < E2E_LOSS_FRACTION * log[0]['main/loss'], [e['main/loss'] for e in log]
    assert log[-1]['val/main/iou/road'] > E2E_MIN_IOU, log[-1]
    assert log[-1]['lr'] == pytest.approx(0.001) and log[0]['lr'] == 0.01
    args = json.load(open(os.path.join(d1, 'args.txt')))
    assert args['model'] == 'basic' and args['input_shape'] == [64, 128]
    # --resume from the middle reaches the same snapshot, bit for bit
    _run([os.path.join(ROOT, 'train_segnet.py')] + common + ['--result_dir', d2, '--resume',
                                                             os.path.join(d1, 'snapshot_iter_20')], ROOT)
    with np.load(os.path.join(d1, 'snapshot_iter_40')) as a, np.load(os.path.join(d2, 'snapshot_iter_40')) as b:
        assert set(a.files) == set(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), k
    # labels_from_segnet.py on the trainer's snapshot predicts what the trainer's validation predicted
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
