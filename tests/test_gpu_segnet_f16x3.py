"""GPU tests of split-plane SegNet-Basic inference (spa_segnet_encode_f16x3 / spa_segnet_decode_f16x3,
SegNetBasic(split_planes=True), labels_from_segnet.py --split_planes, train_segnet.py --val_split_planes): float32
accuracy on the f16 matrix cores.  The reference is float64 on the UNROUNDED float32 operands (the oracle functions of
tests/segnet_ref.py) and the bounds are tests/test_gpu_segnet.py's float32-inference bounds: the mode claims
float32 accuracy, so it is held to what the float32 kernels are held to.  Every layer test prints this mode's worst
error beside the float32 kernel's on the same inputs."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_ref as sref  # noqa: E402
import segnet_train_synth as syn  # noqa: E402
from segnet_ref import (channels_last, classifier, conv_bias, folded, lrn_chainer, nchw64, pool_err,  # noqa: E402
                        random_params, standardise, t64, unpool)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
segnet = importlib.import_module('superpixel-align_amd.segnet')

# Layer values as a fraction of max|ref| (tests/test_gpu_segnet.py's check_pool / decoder bound).
# Measured worst over the layer tests below (dynamic-range cases included): this mode 6.7e-7, the float32 kernels
# 2.3e-6 on the same inputs (conv1 2.5e-7 / 3.9e-7, encoders 6.7e-7 / 2.3e-6, decoder 6.6e-7 / 1.3e-6).
LAYER_TOL = 1e-5
# decode1's probabilities, absolute (tests/test_gpu_segnet.py's).
# Measured worst: this mode 9.8e-7, the float32 kernel 1.5e-6 on the same inputs.
PROB_TOL = 1e-5
# Share of pooling windows the index rule leaves undecided (see check_pool).  The float64 reference alone leaves
# 0 - 1.8e-4 undecided at these shapes with these weights.
EXEMPT_WINDOWS = 1e-3
# Whole network (tests/test_gpu_segnet.py's test_predict_full_size): resized scores, the near-tie band of the labels,
# and the share of pixels that may lie inside that band (the float64 network alone: 6e-4 - 1.0e-3 at smaller sizes).
NET_SCORE_TOL = 1e-4
NET_NEAR = 1e-3
NET_EXEMPT_PIXELS = 1e-2


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


def check_pool(pooled, idx, v, what):
    return sref.check_pool_decided(pooled, idx, v, LAYER_TOL, EXEMPT_WINDOWS, what)


def report(what, e3, e32):
    print('%s: split-plane %.3g, float32 kernel %.3g' % (what, e3, e32))
    if e3 > 2 * e32:
        print('%s: FINDING: the split-plane error is more than twice the float32 kernel\'s' % what)


# ------------------------------------------------------------------------------- the four forms
def run_conv1(eng, img, p, ws=1.0, what='conv1'):
    w, b, w64, b64 = folded(p, 'conv1', ws, ws)
    x = torch.from_numpy(img).cuda()
    pooled, idx = eng.segnet_encode_f16x3(x, w, b, segnet.MEAN, segnet.STD)
    p32, _ = eng.segnet_encode(x, w, b, segnet.MEAN, segnet.STD)
    torch.cuda.synchronize()
    B, _, H, W = img.shape
    assert pooled.shape == (B, 64, H // 2, W // 2) and pooled.is_contiguous(memory_format=torch.channels_last)
    assert idx.dtype == torch.uint8 and idx.shape == pooled.shape
    v = conv_bias(lrn_chainer(t64(standardise(img))), w64, b64)
    e = check_pool(pooled, idx, v, what)
    report(what, e, pool_err(p32, v))
    return e


def run_encoder(eng, x, p, xs=1.0, ws=1.0, what='encoder'):
    """x (B,64,H,W) float32 CPU; the map scaled by xs, the weights by ws, the bias by xs * ws"""
    w, b, w64, b64 = folded(p, 'conv2', ws, xs * ws)
    xd = channels_last(x * xs)
    pooled, idx = eng.segnet_encode_f16x3(xd, w, b)
    p32, _ = eng.segnet_encode(xd, w, b)
    torch.cuda.synchronize()
    v = conv_bias(nchw64(xd), w64, b64)
    e = check_pool(pooled, idx, v, what)
    report(what, e, pool_err(p32, v))
    return e


def device_pool(eng, p, shape, seed, xs=1.0):
    """a pooled map and its indices as this mode's encoder leaves them, the map scaled by xs afterwards (exact)"""
    x = channels_last(torch.randn(shape, generator=torch.Generator().manual_seed(seed)))
    w, b, _, _ = folded(p, 'conv3')
    pooled, idx = eng.segnet_encode_f16x3(x, w, b)
    return (pooled * xs).contiguous(memory_format=torch.channels_last), idx


def run_decoder(eng, p, xs=1.0, ws=1.0, what='decoder'):
    pooled, idx = device_pool(eng, p, (2, 64, 32, 64), 15, xs)
    w, b, w64, b64 = folded(p, 'conv_decode3', ws, xs * ws)
    y = eng.segnet_decode_f16x3(pooled, idx, w, b)
    y32 = eng.segnet_decode(pooled, idx, w, b)
    torch.cuda.synchronize()
    assert y.shape == (2, 64, 32, 64) and y.is_contiguous(memory_format=torch.channels_last)
    ref = conv_bias(unpool(nchw64(pooled), idx.cpu()), w64, b64)
    scale = float(ref.abs().max())
    e, e32 = float((nchw64(y) - ref).abs().max()) / scale, float((nchw64(y32) - ref).abs().max()) / scale
    report(what, e, e32)
    assert e <= LAYER_TOL, '%s: error %.3g of max|ref|' % (what, e)
    return e


def run_decode1(eng, p, xs=1.0, ws=1.0, what='decode1'):
    """the classifier's weight is scaled by 1 / (xs ws) (a power of two: exact), so that the logits keep their size
    and the probabilities stay a sensitive check whatever the operands' scales"""
    pooled, idx = device_pool(eng, p, (2, 64, 32, 48), 17, xs)
    w, b, w64, b64 = folded(p, 'conv_decode1', ws, xs * ws)
    wc, bc, wc64, bc64 = classifier(p, 1.0 / (xs * ws))
    prob = eng.segnet_decode_f16x3(pooled, idx, w, b, wc, bc)
    p32 = eng.segnet_decode(pooled, idx, w, b, wc, bc)
    torch.cuda.synchronize()
    assert prob.shape == (2, 2, 32, 48) and prob.is_contiguous()
    y = conv_bias(unpool(nchw64(pooled), idx.cpu()), w64, b64)
    ref = torch.softmax(F.conv2d(y, wc64[:, :, None, None], bc64), 1)
    e, e32 = float((nchw64(prob) - ref).abs().max()), float((nchw64(p32) - ref).abs().max())
    report(what + ' probabilities', e, e32)
    assert e <= PROB_TOL, '%s: probability error %.3g' % (what, e)
    return e


def test_conv1_against_float64(eng):
    img = np.random.default_rng(11).integers(0, 256, (2, 3, 48, 96)).astype(np.float32)
    run_conv1(eng, img, random_params(10))


@pytest.mark.parametrize('H,W', [(32, 64), (20, 36)])
def test_encoder_64_against_float64(eng, H, W):
    x = torch.randn((2, 64, H, W), generator=torch.Generator().manual_seed(13))
    run_encoder(eng, x, random_params(12), what='encoder (2,64,%d,%d)' % (H, W))


def test_decoder_on_device_pool(eng):
    run_decoder(eng, random_params(14))


def test_decode1_classifier_softmax(eng):
    run_decode1(eng, random_params(16))


# ------------------------------------------------------------------------------- dynamic range
@pytest.mark.parametrize('xs,ws', [(2.0 ** 20, 2.0 ** -12), (2.0 ** -20, 1.0)])
def test_dynamic_range_64(eng, xs, ws):
    """maps at 2^20 with weights at 2^-12, and maps at 2^-20: the per-operand scales keep every plane inside f16's
    range, and the relative bounds are those of the O(1) tests"""
    tag = ' (maps x %g, weights x %g)' % (xs, ws)
    for H, W in ((32, 64), (20, 36)):
        x = torch.randn((2, 64, H, W), generator=torch.Generator().manual_seed(43))
        run_encoder(eng, x, random_params(42), xs, ws, what='encoder (2,64,%d,%d)%s' % (H, W, tag))
    run_decoder(eng, random_params(44), xs, ws, what='decoder' + tag)
    run_decode1(eng, random_params(46), xs, ws, what='decode1' + tag)


@pytest.mark.parametrize('ws', [2.0 ** -12, 2.0 ** 12])
def test_dynamic_range_conv1(eng, ws):
    """conv1's operand is bounded by the LRN; its weights at 2^-12 and 2^12 (bias scaled to match)"""
    img = np.random.default_rng(48).integers(0, 256, (2, 3, 48, 96)).astype(np.float32)
    run_conv1(eng, img, random_params(47), ws, what='conv1 (weights x %g)' % ws)


# ------------------------------------------------------------------------------- all-zero operands
def test_all_zero_operands_give_exact_results(eng):
    p = random_params(50)
    g = torch.Generator().manual_seed(51)
    x = channels_last(torch.randn((2, 64, 20, 36), generator=g))
    w, b, _, _ = folded(p, 'conv2')
    relu_b = torch.relu(b)[None, :, None, None]
    for xin, win in ((torch.zeros_like(x), w), (x, torch.zeros_like(w)), (torch.zeros_like(x), torch.zeros_like(w))):
        pooled, idx = eng.segnet_encode_f16x3(xin, win, b)
        assert torch.equal(pooled, relu_b.expand_as(pooled)) and int(idx.max()) == 0
    img = (torch.rand((2, 3, 32, 48), generator=g) * 255).cuda()
    w1, b1, _, _ = folded(p, 'conv1')
    pooled, idx = eng.segnet_encode_f16x3(img, torch.zeros_like(w1), b1, segnet.MEAN, segnet.STD)
    assert torch.equal(pooled, torch.relu(b1)[None, :, None, None].expand_as(pooled)) and int(idx.max()) == 0
    # decoder: y == bias
    h = channels_last(torch.rand((2, 64, 10, 18), generator=g))
    hi = channels_last(torch.randint(0, 4, (2, 64, 10, 18), generator=g, dtype=torch.uint8))
    wd, bd, _, _ = folded(p, 'conv_decode2')
    for hin, win in ((torch.zeros_like(h), wd), (h, torch.zeros_like(wd))):
        y = eng.segnet_decode_f16x3(hin, hi, win, bd)
        assert torch.equal(y, bd[None, :, None, None].expand_as(y))
    # decode1: the classifier of the bias at every pixel
    h = channels_last(torch.rand((2, 64, 8, 16), generator=g))
    hi = channels_last(torch.randint(0, 4, (2, 64, 8, 16), generator=g, dtype=torch.uint8))
    w1d, b1d, _, b64 = folded(p, 'conv_decode1')
    wc, bc, wc64, bc64 = classifier(p)
    want = torch.softmax(wc64 @ b64 + bc64, 0)
    for hin, win in ((torch.zeros_like(h), w1d), (h, torch.zeros_like(w1d))):
        prob = eng.segnet_decode_f16x3(hin, hi, win, b1d, wc, bc)
        assert torch.equal(prob, prob[:1, :, :1, :1].expand_as(prob))            # the same bits at every pixel
        assert float((prob[0, :, 0, 0].cpu().double() - want).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------- writes, through the C entry points
@pytest.mark.parametrize('form', ['conv1', 'enc', 'dec', 'dec1'])
def test_outputs_fully_written_and_bounded(eng, form):
    sref.check_outputs_written(eng, '_f16x3', form)


# ------------------------------------------------------------------------------- determinism
def test_same_bits_twice_and_on_a_second_context(eng):
    p = random_params(60)
    model = segnet.SegNetBasic(p, engine=eng, split_planes=True)
    imgs = torch.from_numpy(np.random.default_rng(61).integers(0, 256, (2, 3, 48, 80)).astype(np.float32)).cuda()
    t1, t2, t3 = [], [], []
    a = model.forward(imgs, trace=t1)
    b = model.forward(imgs, trace=t2)
    engine = importlib.import_module('superpixel-align_amd.engine')
    e2 = engine.Engine()
    try:
        c = segnet.SegNetBasic(p, engine=e2, split_planes=True).forward(imgs, trace=t3)
        torch.cuda.synchronize()
    finally:
        e2.close()
    assert torch.equal(a, b) and torch.equal(a, c)
    for (x1, i1), (x2, i2), (x3, i3) in zip(t1, t2, t3):
        assert torch.equal(x1, x2) and torch.equal(i1, i2) and torch.equal(x1, x3) and torch.equal(i1, i3)


def _positions(own, other_a, other_b):
    """the batches (own alone, own first of three, own last of three) and own's position in each"""
    return [(own, 0), (torch.cat([own, other_a, other_b]), 0), (torch.cat([other_a, other_b, own]), 2)]


def test_determinism_batch_position(eng):
    """An image's outputs have the same bits alone, first of three and last of three, beside neighbours of much larger
    magnitude (maps x 2^6; for conv1 a dark image, values 0..31, beside full-range ones): a per-batch activation scale
    would give the image other h / l planes."""
    p = random_params(62)
    g = torch.Generator().manual_seed(63)
    # conv1
    dark = torch.randint(0, 32, (1, 3, 48, 80), generator=g).float().cuda()
    full = [torch.randint(0, 256, (1, 3, 48, 80), generator=g).float().cuda() for _ in range(2)]
    full[0][0, :, :8, :8] = 255.0
    w, b, _, _ = folded(p, 'conv1')
    outs = [(eng.segnet_encode_f16x3(x.contiguous(), w, b, segnet.MEAN, segnet.STD), k)
            for x, k in _positions(dark, *full)]
    for (pooled, idx), k in outs[1:]:
        assert torch.equal(pooled[k], outs[0][0][0][0]) and torch.equal(idx[k], outs[0][0][1][0]), 'conv1'
    # encoder, then decoder and decode1 on its pools
    own = torch.randn((1, 64, 32, 48), generator=g)
    big = [torch.randn((1, 64, 32, 48), generator=g) * 64.0 for _ in range(2)]
    w, b, _, _ = folded(p, 'conv2')
    wd, bd, _, _ = folded(p, 'conv_decode2')
    w1, b1, _, _ = folded(p, 'conv_decode1')
    wc, bc, _, _ = classifier(p)
    res = []
    for x, k in _positions(own, *big):
        pooled, idx = eng.segnet_encode_f16x3(channels_last(x), w, b)
        y = eng.segnet_decode_f16x3(pooled, idx, wd, bd)
        prob = eng.segnet_decode_f16x3(pooled, idx, w1, b1, wc, bc)
        res.append((pooled[k], idx[k], y[k], prob[k]))
    torch.cuda.synchronize()
    for r in res[1:]:
        for a, c, what in zip(res[0], r, ('encoder pooled', 'encoder indices', 'decoder', 'decode1 probabilities')):
            assert torch.equal(a, c), what
    # the network
    model = segnet.SegNetBasic(p, engine=eng, split_planes=True)
    dark = torch.randint(0, 32, (1, 3, 64, 128), generator=g).float().cuda()
    full = [torch.randint(0, 256, (1, 3, 64, 128), generator=g).float().cuda() for _ in range(2)]
    nets = []
    for x, k in _positions(dark, *full):
        trace = []
        prob = model.forward(x.contiguous(), trace=trace)
        nets.append([prob[k]] + [t[k] for pair in trace for t in pair])
    torch.cuda.synchronize()
    for r in nets[1:]:
        for a, c in zip(nets[0], r):
            assert torch.equal(a, c)


# ------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(eng):
    sref.check_inference_refusals(eng, '_f16x3')


# ------------------------------------------------------------------------------- whole network
def test_predict_full_size(eng):
    p = random_params(19)
    g = np.random.default_rng(20)
    img = g.integers(0, 256, (2, 3, 512, 1024)).astype(np.float32)
    model = segnet.SegNetBasic(p, pred_shape=(1024, 2048), engine=eng, split_planes=True)
    out = model.predict(img, return_score=True)
    out32 = segnet.SegNetBasic(p, pred_shape=(1024, 2048), engine=eng).predict(img)
    trace = []
    model.forward(torch.from_numpy(img).cuda(), trace=trace)         # the same launches: the indices predict used
    # the device's pooling indices are required to be decided_windows' (LAYER_TOL max|y|) in every decided window
    ref = sref.forward64(p, t64(standardise(img)), [i for _, i in trace], sref.decided_indices, LAYER_TOL)[0].numpy()
    for bi in range(2):
        label, score = out[bi]
        assert label.shape == (1024, 2048) and score.shape == (2, 1024, 2048) and score.dtype == np.float32
        # the float64 probabilities through the same (host) resize: the remaining difference is the network's rounding
        want = segnet.resize_bilinear_pil(ref[bi].astype(np.float32), (1024, 2048))
        err = float(np.abs(score - want).max())
        near = np.abs(want[1] - want[0]) < NET_NEAR
        print('image %d: score error %.3g, pixels inside |p1 - p0| < %g: %.3g, labels differing from the float32 '
              'network\'s: %.3g' % (bi, err, NET_NEAR, float(near.mean()), float((label != out32[bi]).mean())))
        assert err <= NET_SCORE_TOL
        assert float(near.mean()) <= NET_EXEMPT_PIXELS
        assert np.array_equal(label[~near], np.argmax(want, 0)[~near])


class _Spy(object):
    """an engine that counts the calls of its segnet_* methods"""

    def __init__(self, eng):
        self._eng = eng
        self.calls = {}

    def __getattr__(self, name):
        attr = getattr(self._eng, name)
        if not name.startswith('segnet_'):
            return attr

        def counted(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return attr(*a, **k)
        return counted


def test_default_untouched_and_flag_takes_the_f16x3_stages(eng):
    p = random_params(42)
    x = torch.from_numpy(np.random.default_rng(43).integers(0, 256, (2, 3, 64, 128)).astype(np.float32)).cuda()
    a = segnet.SegNetBasic(p, engine=eng).forward(x)
    b = segnet.SegNetBasic(p, engine=eng, split_planes=False).forward(x)
    spy = _Spy(eng)
    c = segnet.SegNetBasic(p, engine=spy, split_planes=True).forward(x)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert spy.calls == {'segnet_encode_f16x3': 4, 'segnet_decode_f16x3': 4}
    assert c.shape == a.shape and c.dtype == a.dtype and bool(torch.isfinite(c).all())
    spy32 = _Spy(eng)
    segnet.SegNetBasic(p, engine=spy32).forward(x)
    assert spy32.calls == {'segnet_encode': 4, 'segnet_decode': 4}


# ------------------------------------------------------------------------------- end to end
# The float32 end-to-end test's settings and bounds (tests/test_gpu_segnet_train.py).
E2E_ITERS = 40
E2E_MIN_IOU = 0.6
# Split-plane masks against the float32 masks of the same snapshot: the fraction of pixels that agree.  Both are
# float32-accurate, so a pixel can differ only where p1 - p0 is within the two paths' rounding (1e-5) of zero.
# Measured: 1.0 (every pixel) over the three 64 x 128 validation images; the bound leaves room for 24 pixels.
E2E_MIN_AGREEMENT = 0.999
REF_KEYS = ['img_fn', 'label_fn', 'road_iou', 'non_road_iou', 'precision', 'recall', 'TP', 'FP', 'FN', 'param_dir',
            'iteration', 'gpu', 'img_zip_fn', 'label_zip_fn', 'out_dir', 'start_index', 'end_index', 'soft_label',
            'eval_shape', 'save_each', 'train_args']


def test_train_then_label_split_planes_end_to_end(tmp_path):
    z = syn.write(str(tmp_path / 'data'), 8, 3, 64, 128)
    common = syn.train_args(z, E2E_ITERS, 20, 10, extra=['--decay_iteration', '30'])
    d1, d2 = str(tmp_path / 'run'), str(tmp_path / 'run_val_split')
    syn.run_python([os.path.join(ROOT, 'train_segnet.py')] + common + ['--result_dir', d1], ROOT)
    syn.run_python([os.path.join(ROOT, 'train_segnet.py')] + common + ['--result_dir', d2, '--val_split_planes'], ROOT)
    # validation on split planes: logged, recorded in args.txt only when given, and without influence on the training
    log1, log2 = (json.load(open(os.path.join(d, 'log'))) for d in (d1, d2))
    print('val/main/iou/road: float32 validation %.4f, split-plane validation %.4f'
          % (log1[-1]['val/main/iou/road'], log2[-1]['val/main/iou/road']))
    assert log2[-1]['val/main/iou/road'] > E2E_MIN_IOU, log2[-1]
    a1, a2 = (json.load(open(os.path.join(d, 'args.txt'))) for d in (d1, d2))
    assert 'val_split_planes' not in a1 and a2['val_split_planes'] is True
    with np.load(os.path.join(d1, 'snapshot_iter_%d' % E2E_ITERS)) as s1, \
            np.load(os.path.join(d2, 'snapshot_iter_%d' % E2E_ITERS)) as s2:
        keys = [k for k in s1.files if k.startswith(segnet.PREFIX)]
        assert len(keys) >= 8 * 5 + 2 and sorted(s1.files) == sorted(s2.files)
        for k in keys:
            assert np.array_equal(s1[k], s2[k]), k
    # labelling
    label_cmd = [os.path.join(ROOT, 'labels_from_segnet.py'), '--param_dir', d1, '--iteration', str(E2E_ITERS),
                 '--img_zip_fn', z[2], '--label_zip_fn', z[3], '--start_index', '0', '--end_index', '3',
                 '--eval_shape', '64', '128', '--no_figure']
    out_s, out_f = str(tmp_path / 'labels_split'), str(tmp_path / 'labels')
    syn.run_python(label_cmd + ['--out_dir', out_s, '--split_planes'], ROOT)
    syn.run_python(label_cmd + ['--out_dir', out_f], ROOT)
    lines = [json.loads(l) for l in open(os.path.join(out_s, 'result.json')) if l.strip()]
    assert len(lines) == 3
    TP = FP = FN = 0
    agree, total = 0, 0
    for line in lines:
        assert list(line) == REF_KEYS + ['split_planes'] and line['split_planes'] is True
        assert line['save_each'] is True and line['eval_shape'] == [64, 128]
        base = os.path.splitext(os.path.basename(line['img_fn']))[0]
        mask = np.load(os.path.join(out_s, base + '.npy'))
        assert mask.dtype == np.bool_ and mask.shape == (64, 128)
        assert np.array_equal(np.load(os.path.join(out_s, base + '_scores.npy')), mask)
        m32 = np.load(os.path.join(out_f, base + '.npy'))
        agree += int((mask == m32).sum())
        total += mask.size
        TP, FP, FN = TP + line['TP'], FP + line['FP'], FN + line['FN']
    iou = TP / float(TP + FP + FN)
    print('split-plane labels: road IoU %.4f, agreement with the float32 masks %.6f' % (iou, agree / float(total)))
    assert iou > E2E_MIN_IOU
    assert agree / float(total) >= E2E_MIN_AGREEMENT
    for line in (json.loads(l) for l in open(os.path.join(out_f, 'result.json')) if l.strip()):
        assert list(line) == REF_KEYS                                  # float32 lines: the reference's keys only
    # the CLI refuses the flag with bf16 and writes nothing
    out_r = str(tmp_path / 'labels_refused')
    r = subprocess.run([sys.executable] + label_cmd + ['--out_dir', out_r, '--split_planes', '--dtype', 'bf16'],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'split_planes' in r.stderr and not os.path.exists(out_r)
    # save_labels(save_each=False, split_planes=True) returns the float32 scores at eval_shape
    sys.path.insert(0, ROOT)
    lfs = importlib.import_module('labels_from_segnet')
    res = lfs.save_labels(d1, E2E_ITERS, 0, z[2], z[3], str(tmp_path / 'mem'), 1, 2, False, [64, 128],
                          save_each=False, figure=False, split_planes=True)
    assert len(res) == 2
    for k, v in res.items():
        if k.endswith('_scores'):
            assert v.dtype == np.float32 and v.shape == (2, 64, 128)
            assert np.array_equal(res[k[:-len('_scores')]], np.argmax(v, 0).astype(bool))
