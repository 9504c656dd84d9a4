"""GPU tests of bf16 SegNet-Basic inference (spa_segnet_encode_bf16 / spa_segnet_decode_bf16, SegNetBasic(dtype='bf16'),
labels_from_segnet.py --dtype bf16): each of the four layer forms against the float64 restatement of
tests/segnet_ref.py on the kernel's own bf16 operands, full and bounded writes, determinism across batch positions,
the refusals, the whole network at the training size against a restatement that rounds every layer's operands to bf16,
the fp32 default left as it was, and the labelling driver end to end on a synthetic zipped dataset."""
import importlib
import json
import os
import shutil
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
F = torch.nn.functional
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_ref as sref  # noqa: E402
import segnet_train_synth as syn  # noqa: E402
from segnet_ref import channels_last, conv7, conv_bias, nchw64, r16, random_params, windows  # noqa: E402

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


def folded(p, name):
    """(device packed float32 weight, device bias, float64 (64,Cin,7,7) bf16 weight operand, float64 bias)"""
    return sref.folded(p, name, operand=r16)


def conv1_operand(eng, img):
    """conv1's float32 input as the kernels load it, checked against the float64 restatement, (B,3,H,W) on the CPU"""
    return sref.nchw(sref.conv1_operand(eng, img, check=True)).contiguous()


def check_pool(pooled, idx, ref64, what):
    return sref.check_pool_near_ties(pooled, idx, ref64, LAYER_TOL, what)


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
    ref = torch.relu(conv_bias(r16(conv1_operand(eng, img)), w64, b64))
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
    ref = torch.relu(conv_bias(r16(x.cpu()), w64, b64))
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
    ref = conv_bias(st.unpool_ref(r16(h.cpu()), idx.cpu().long()), w64, b64)
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
    y = conv_bias(st.unpool_ref(r16(h.cpu()), idx.cpu().long()), w64, b64)
    z = F.conv2d(y, torch.from_numpy(wc).double()[:, :, None, None], torch.from_numpy(bc).double())
    ref = torch.softmax(z, 1)
    e = float((prob.cpu().double() - ref).abs().max())
    print('decode1 %s: probability error %.3g' % (shape, e))
    assert e <= PROB_TOL


# ------------------------------------------------------------------------------- writes, through the C entry points
@pytest.mark.parametrize('form', ['conv1', 'enc', 'dec', 'dec1'])
def test_outputs_fully_written_and_bounded(eng, form):
    sref.check_outputs_written(eng, '_bf16', form)


# ------------------------------------------------------------------------------- determinism
def test_determinism_batch_position(eng):
    g = np.random.default_rng(41)
    model = segnet.SegNetBasic(random_params(40), engine=eng, dtype='bf16')
    imgs = torch.from_numpy(g.integers(0, 256, (3, 3, 48, 80)).astype(np.float32)).cuda()
    sref.check_batch_position(model, imgs, layers=True)             # every layer's output repeats bit for bit too


# ------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(eng):
    sref.check_inference_refusals(eng, '_bf16')


# ------------------------------------------------------------------------------- whole network
# conv1's bf16 operand is the bf16 rounding of the float32 training kernel's operand (sref.conv1_operand) bit for bit, in
# every call and at every grid size (tests/test_gpu_segnet_exact.py; the bf16 files are built without packed float32
# instructions in the LRN).  So the full-size conv1 check is the other layers': no output beyond
# LAYER_TOL.  Before that build these two were 5e-3 and 2e-3 and absorbed operands one bf16 step off.
CONV1_FLIP_FRACTION = 0.0
CONV1_FLIP_TOL = LAYER_TOL
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
    ref = torch.relu(conv_bias(r16(conv1_operand(eng, torch.from_numpy(img))), w64, b64))
    err = (nchw64(trace[0][0]) - windows(ref).max(-1).values).abs() / float(ref.abs().max())
    flips = float((err > LAYER_TOL).double().mean())
    print('conv1 at full size: %.3g of the outputs beyond LAYER_TOL, worst %.3g of max|ref|' % (flips, float(err.max())))
    assert flips <= CONV1_FLIP_FRACTION and float(err.max()) <= CONV1_FLIP_TOL
    del ref, err
    worst = 0.0
    for name, (pooled, idx), (h, _) in zip(segnet.ENCODERS[1:], trace[1:], trace):
        _, _, w64, b64 = folded(p, name)
        ref = torch.relu(conv_bias(r16(h.cpu()), w64, b64))
        worst = max(worst, check_pool(pooled, idx, ref, name))
    hd = trace[-1][0]
    for name, (_, idx) in zip(segnet.DECODERS, trace[::-1]):
        w, b, w64, b64 = folded(p, name)
        ref = conv_bias(st.unpool_ref(r16(hd.cpu()), idx.cpu().long()), w64, b64)
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


def _files(d):
    out = {}
    for fn in sorted(os.listdir(d)):
        with open(os.path.join(d, fn), 'rb') as f:
            out[fn] = f.read()
    return out


def test_train_then_label_bf16_end_to_end(tmp_path):
    z = syn.write(str(tmp_path / 'data'), 8, 3, 64, 128)
    common = syn.train_args(z, E2E_ITERS, 20, 10, extra=['--decay_iteration', '30'])
    d1 = str(tmp_path / 'run')
    syn.run_python([os.path.join(ROOT, 'train_segnet.py')] + common + ['--result_dir', d1], ROOT)
    label_cmd = [os.path.join(ROOT, 'labels_from_segnet.py'), '--param_dir', d1, '--iteration', str(E2E_ITERS),
                 '--img_zip_fn', z[2], '--label_zip_fn', z[3], '--start_index', '0', '--end_index', '3',
                 '--eval_shape', '64', '128', '--no_figure']
    out_b, out_f = str(tmp_path / 'labels_bf16'), str(tmp_path / 'labels')
    syn.run_python(label_cmd + ['--out_dir', out_b, '--dtype', 'bf16'], ROOT)
    syn.run_python(label_cmd + ['--out_dir', out_f], ROOT)
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
    syn.run_python(label_cmd + ['--out_dir', out_f, '--dtype', 'fp32'], ROOT)
    assert _files(out_f) == _files(out_f + '_default')
