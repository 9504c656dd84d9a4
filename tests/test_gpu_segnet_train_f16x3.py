"""GPU tests of SegNet-Basic training at float32 accuracy on the f16 matrix cores (csrc/spa_segnet_train_f16x3.hip,
SegNetTrainer(..., split_planes=True), train_segnet.py --split_planes): the eight pass forms against float64 torch
convolutions of the UNROUNDED float32 operands within the float32 forms' bounds, also at extreme dynamic range, exact
zeros, the BatchNorm partial sums, NaN-poisoned outputs with a guard past the end, the float32 entry points' refusal
codes, bit-identical repeats within and across contexts, one whole step against the float64 restatement within the
float32 step's bounds, and train_segnet.py --split_planes -> --resume -> labels_from_segnet.py end to end.
The pass checks are the shared bodies of tests/segnet_ref.py, called with this file's family and bounds."""
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_ref as sref  # noqa: E402
import segnet_train_synth as syn  # noqa: E402

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
# split-plane entry points; float32 operands enter the reference unrounded; conv1's input is the float32 kernels' own
# operand (not re-checked: the dynamic-range images are off the 0..255 scale)
MODE = dict(family='_f16x3', operand=sref.d64)
CONV1 = dict(device_conv1=True, check_conv1=False)

# dynamic range: inputs at 2^20, output gradients at 2^-30, weights at 2^-12 (f16 spans 2^-24 .. 2^16)
X_SCALE, DY_SCALE, W_SCALE = 2.0 ** 20, 2.0 ** -30, 2.0 ** -12


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


def check_forward(eng, shape, seed, **scales):
    return sref.check_forward(eng, shape, seed, fwd_tol=FWD_TOL, bn_tol=BN_TOL, **MODE, **CONV1, **scales)


def check_dgrad(eng, shape, seed, **scales):
    return sref.check_dgrad(eng, shape, seed, fwd_tol=FWD_TOL, **MODE, **scales)


def check_wgrad(eng, shape, seed, **scales):
    return sref.check_wgrad(eng, shape, seed, wgrad_tol=WGRAD_TOL, **MODE, **CONV1, **scales)


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_forms_and_bn_sums(eng, shape):
    print('f16x3 forward %s: worst %.3g' % (shape, check_forward(eng, shape, 1)))


@pytest.mark.parametrize('shape', SHAPES)
def test_dgrad_forms(eng, shape):
    print('f16x3 dgrad %s: worst %.3g' % (shape, check_dgrad(eng, shape, 2)))


@pytest.mark.parametrize('shape', SHAPES)
def test_wgrad_forms(eng, shape):
    print('f16x3 wgrad %s: worst %.3g' % (shape, check_wgrad(eng, shape, 3)))


def test_wgrad_decode1_full_size(eng):
    sref.check_wgrad_decode1_full_size(eng, big_tol=WGRAD_BIG_TOL, label='f16x3', **MODE)


@pytest.mark.parametrize('shape', [(2, 48, 80), (2, 6, 10)])
def test_dynamic_range(eng, shape):
    """inputs at 2^20, dy at 2^-30, weights at 2^-12: the per-tensor scales keep every plane inside f16's range"""
    e = [check_forward(eng, shape, 11, xs=X_SCALE, ws=W_SCALE),
         check_dgrad(eng, shape, 12, dys=DY_SCALE, ws=W_SCALE),
         check_wgrad(eng, shape, 13, xs=X_SCALE, dys=DY_SCALE)]
    print('f16x3 dynamic range %s: forward %.3g, dgrad %.3g, wgrad %.3g' % ((shape,) + tuple(e)))


def test_all_zero_operands_give_exact_zeros(eng):
    B, H, W = 2, 32, 64
    img, x, h, idx, dy, w1, w64 = sref.inputs(B, H, W, 21)
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
    out, buf = sref.poisoned((1, 25, 32, 64))
    dw, dbuf = sref.poisoned((49, 64, 64))
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
    img, x, h, idx, dy, w1, w64 = sref.inputs(B, H, W, 31)
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
    r = sref.step_against_float64(eng, dict(split_planes=True))
    loss, l64, worst, es = r['loss'], r['l64'], r['updates'], r['stats']
    el = abs(loss - l64) / abs(l64)
    ku, ks = max(worst, key=worst.get), max(es, key=es.get)
    print('f16x3 step: loss error %.3g, worst update error %.3g (%s), worst running statistic error %.3g (%s)'
          % (el, worst[ku], ku, es[ks], ks))
    assert el < LOSS_TOL, 'loss %.9g vs float64 %.9g' % (loss, l64)
    assert worst[ku] < STEP_TOL, '%s: update error %.3g' % (ku, worst[ku])
    assert es[ks] < STAT_TOL, '%s: running statistic error %.3g' % (ks, es[ks])


def test_split_plane_step_repeats_bit_for_bit(eng):
    sref.check_step_repeats(eng, split_planes=True)


# ------------------------------------------------------------------------------- end to end
# The float32 end-to-end test's settings and bounds (tests/test_gpu_segnet_train.py).
E2E_ITERS = 40
E2E_LOSS_FRACTION = 0.35
E2E_MIN_IOU = 0.6


def test_train_split_planes_then_label_end_to_end(tmp_path):
    z = syn.write(str(tmp_path / 'data'), 8, 3, 64, 128)
    common = syn.train_args(z, E2E_ITERS, 20, 10, extra=['--decay_iteration', '30'])
    d1, d2 = str(tmp_path / 'run'), str(tmp_path / 'resumed')
    script = os.path.join(ROOT, 'train_segnet.py')
    syn.run_python([script, '--split_planes'] + common + ['--result_dir', d1], ROOT)
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
    syn.run_python([script, '--split_planes'] + common + ['--result_dir', d2, '--resume', snap20], ROOT)
    with np.load(os.path.join(d1, 'snapshot_iter_40')) as a, np.load(os.path.join(d2, 'snapshot_iter_40')) as b:
        assert set(a.files) == set(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), k
    # labels_from_segnet.py (save_labels) reads the split-plane snapshot and predicts what the validation predicted
    out = str(tmp_path / 'labels')
    syn.run_python([os.path.join(ROOT, 'labels_from_segnet.py'), '--param_dir', d1, '--iteration', str(E2E_ITERS),
          '--img_zip_fn', z[2], '--label_zip_fn', z[3], '--out_dir', out, '--start_index', '0', '--end_index', '3',
          '--eval_shape', '64', '128', '--no_figure'], ROOT)
    res = [json.loads(l) for l in open(os.path.join(out, 'result.json')) if l.strip()]
    FP = sum(r['FP'] for r in res)
    FN = sum(r['FN'] for r in res)
    TP = sum(r['TP'] for r in res)
    assert (FP, FN) == (log[-1]['val_/main/FP'], log[-1]['val_/main/FN'])
    assert TP / float(TP + FP + FN) == log[-1]['val/main/iou/road']
