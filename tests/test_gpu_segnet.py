"""GPU tests of SegNet-Basic inference (labels_from_segnet.py) on libspalign's kernels: every layer kind against the
float64 restatement of models/segnet_basic.py in tests/segnet_ref.py (torch CPU ops, Chainer's LRN formula), the Pillow
BILINEAR score resize bit for bit, the whole predict at the training size, determinism across batch sizes, the
refusals, and the labels_from_segnet.py driver end to end on a synthetic zipped dataset."""
import ctypes
import importlib
import json
import os
import subprocess
import sys
import zipfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_ref as sref  # noqa: E402
import segnet_train_synth as syn  # noqa: E402
from segnet_ref import bn_conv, classify, lrn_chainer, nchw64, random_params, standardise, t64, unpool  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
segnet = importlib.import_module('superpixel-align_amd.segnet')

LAYER_TOL = 1e-5          # layer values and the pooling near-tie band, as a fraction of max|ref|
PROB_TOL = 1e-5           # decode1's probabilities, absolute


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


# ------------------------------------------------------------------------------- layers
def test_encoder_conv1_lrn(eng):
    p = random_params(10)
    g = np.random.default_rng(11)
    img = g.integers(0, 256, (2, 3, 48, 96)).astype(np.float32)
    w, b = sref.folded(p, 'conv1')[:2]
    pooled, idx = eng.segnet_encode(torch.from_numpy(img).cuda(), w, b, segnet.MEAN, segnet.STD)
    torch.cuda.synchronize()
    assert pooled.shape == (2, 64, 24, 48) and pooled.is_contiguous(memory_format=torch.channels_last)
    ref64 = torch.relu(bn_conv(p, 'conv1', lrn_chainer(t64(standardise(img)))))
    sref.check_pool_near_ties(pooled, idx, ref64, LAYER_TOL, 'conv1')


@pytest.mark.parametrize('H,W', [(32, 64), (20, 36)])
def test_encoder_64(eng, H, W):
    p = random_params(12)
    x = torch.randn((3, 64, H, W), generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    xd = x.float().cuda().contiguous(memory_format=torch.channels_last)
    w, b = sref.folded(p, 'conv2')[:2]
    pooled, idx = eng.segnet_encode(xd, w, b)
    torch.cuda.synchronize()
    ref64 = torch.relu(bn_conv(p, 'conv2', xd.cpu().double()))
    sref.check_pool_near_ties(pooled, idx, ref64, LAYER_TOL, 'encoder (3,64,%d,%d)' % (H, W))


def test_decoder_on_device_pool(eng):
    p = random_params(14)
    x = torch.randn((2, 64, 32, 64), generator=torch.Generator().manual_seed(15)).cuda().contiguous(
        memory_format=torch.channels_last)
    w2, b2 = sref.folded(p, 'conv3')[:2]
    pooled, idx = eng.segnet_encode(x, w2, b2)
    w, b = sref.folded(p, 'conv_decode3')[:2]
    y = eng.segnet_decode(pooled, idx, w, b)
    torch.cuda.synchronize()
    assert y.shape == (2, 64, 32, 64) and y.is_contiguous(memory_format=torch.channels_last)
    ref64 = bn_conv(p, 'conv_decode3', unpool(nchw64(pooled), idx.cpu()))
    assert float((nchw64(y) - ref64).abs().max()) <= LAYER_TOL * float(ref64.abs().max())


def test_decode1_classifier_softmax(eng):
    p = random_params(16)
    x = torch.randn((2, 64, 32, 48), generator=torch.Generator().manual_seed(17)).cuda().contiguous(
        memory_format=torch.channels_last)
    we, be = sref.folded(p, 'conv4')[:2]
    pooled, idx = eng.segnet_encode(x, we, be)
    w, b = sref.folded(p, 'conv_decode1')[:2]
    wc, bc = segnet.fold_bn(p)['conv_classifier']
    prob = eng.segnet_decode(pooled, idx, w, b, torch.from_numpy(wc).cuda(), torch.from_numpy(bc).cuda())
    torch.cuda.synchronize()
    assert prob.shape == (2, 2, 32, 48) and prob.is_contiguous()
    ref64 = classify(p, bn_conv(p, 'conv_decode1', unpool(nchw64(pooled), idx.cpu())))
    assert float((nchw64(prob) - ref64).abs().max()) <= PROB_TOL


@pytest.mark.parametrize('src,dst', [((16, 32), (32, 64)), ((16, 32), (37, 83)), ((16, 32), (16, 32))])
def test_score_kernel_matches_pillow(eng, src, dst):
    from PIL import Image
    g = torch.Generator().manual_seed(18)
    z = torch.randn((3, 2) + src, generator=g)
    z[:, :, :4, :4] = 0.0                                           # exact ties: class 0
    prob = torch.softmax(z, 1).cuda().contiguous()
    mask, sc = eng.segnet_score(prob, dst, want_scores=True)
    torch.cuda.synchronize()
    ph = prob.cpu().numpy()
    for bi in range(3):
        want = np.stack([np.asarray(Image.fromarray(c, mode='F').resize(dst[::-1], Image.BILINEAR), np.float32)
                         for c in ph[bi]])
        assert np.array_equal(sc[bi].cpu().numpy(), want)
        assert np.array_equal(mask[bi].cpu().numpy(), np.argmax(want, 0).astype(np.uint8))


# ------------------------------------------------------------------------------- whole network
def test_predict_full_size(eng):
    p = random_params(19)
    g = np.random.default_rng(20)
    img = g.integers(0, 256, (2, 3, 512, 1024)).astype(np.float32)
    model = segnet.SegNetBasic(p, pred_shape=(1024, 2048), engine=eng)
    out = model.predict(img, return_score=True)
    trace = []
    model.forward(torch.from_numpy(img).cuda(), trace=trace)         # the same launches: the indices predict used
    # the device's pooling indices are required equal outside near-ties (LAYER_TOL max|y|) and taken inside them
    ref64 = sref.forward64(p, t64(standardise(img)), [i for _, i in trace], sref.near_tie_indices, LAYER_TOL)[0].numpy()
    for bi in range(2):
        label, score = out[bi]
        assert label.shape == (1024, 2048) and score.shape == (2, 1024, 2048) and score.dtype == np.float32
        # the float64 probabilities through the same (host) resize: the remaining difference is the network's rounding
        want = segnet.resize_bilinear_pil(ref64[bi].astype(np.float32), (1024, 2048))
        assert float(np.abs(score - want).max()) <= 1e-4
        near = np.abs(want[1] - want[0]) < 1e-3
        assert np.array_equal(label[~near], np.argmax(want, 0)[~near])


def test_determinism_batch_position(eng):
    g = np.random.default_rng(22)
    model = segnet.SegNetBasic(random_params(21), engine=eng)
    sref.check_batch_position(model, torch.from_numpy(g.integers(0, 256, (3, 3, 64, 128)).astype(np.float32)).cuda())


# ------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(eng):
    sref.check_inference_refusals(eng, '')
    # score: a downscale
    prob = torch.zeros((1, 2, 32, 32), device='cuda')
    mask = torch.full((16 * 64,), 9, dtype=torch.uint8, device='cuda')
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = eng._lib.spa_segnet_score(eng._ctx, ctypes.c_void_p(prob.data_ptr()), 1, 32, 32, 16, 64,
                                   ctypes.c_void_p(mask.data_ptr()), None, s)
    torch.cuda.synchronize()
    assert rc == -1 and bool((mask == 9).all())


# ------------------------------------------------------------------------------- labels_from_segnet.py end to end
@pytest.fixture(scope='module')
def e2e(tmp_path_factory):
    d = tmp_path_factory.mktemp('segnet_e2e')
    g = np.random.default_rng(23)
    keys = ['frankfurt_000000_000294', 'lindau_000001_000019']
    img_zip, label_zip = str(d / 'img.zip'), str(d / 'label.zip')
    labels = {}
    with zipfile.ZipFile(img_zip, 'w') as zi, zipfile.ZipFile(label_zip, 'w') as zl:
        for k in keys:
            city = k.split('_')[0]
            yy, xx = np.mgrid[0:1024, 0:2048]
            img = np.stack([(xx // 8 + yy // 4) % 256, (yy // 3) % 256, g.integers(0, 256, (1024, 2048))], -1)
            zi.writestr('leftImg8bit/val/%s/%s_leftImg8bit.png' % (city, k), syn.png(img.astype(np.uint8)))
            lab = np.where(yy > 600, 7, g.integers(0, 12, (1024, 2048))).astype(np.uint8)
            labels[k] = np.where(lab <= 6, -1, np.where(lab == 7, 1, 0))
            zl.writestr('gtFine/val/%s/%s_gtFine_labelIds.png' % (city, k), syn.png(lab))
    param_dir = d / 'run'
    param_dir.mkdir()
    with open(str(param_dir / 'args.txt'), 'w') as f:
        json.dump({'model': 'basic', 'input_shape': [512, 1024], 'batchsize': 4}, f)
    p = random_params(24)
    with open(str(param_dir / 'snapshot_iter_2000'), 'wb') as f:
        np.savez(f, **{segnet.PREFIX + k: v for k, v in p.items()})
    return dict(dir=d, keys=keys, img_zip=img_zip, label_zip=label_zip, labels=labels, param_dir=str(param_dir))


def test_labels_from_segnet_cli(e2e):
    out = str(e2e['dir'] / 'out')
    cmd = [sys.executable, os.path.join(ROOT, 'labels_from_segnet.py'), '--param_dir', e2e['param_dir'],
           '--iteration', '2000', '--gpu', '-1', '--img_zip_fn', e2e['img_zip'], '--label_zip_fn', e2e['label_zip'],
           '--out_dir', out, '--start_index', '0', '--end_index', '2', '--no_figure', '--batchsize', '2']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in open(os.path.join(out, 'result.json'))]
    assert len(lines) == 2
    keys = ['img_fn', 'label_fn', 'road_iou', 'non_road_iou', 'precision', 'recall', 'TP', 'FP', 'FN', 'param_dir',
            'iteration', 'gpu', 'img_zip_fn', 'label_zip_fn', 'out_dir', 'start_index', 'end_index', 'soft_label',
            'eval_shape', 'save_each', 'train_args']
    for line, k in zip(lines, e2e['keys']):
        assert list(line) == keys
        assert line['gpu'] == -1 and line['eval_shape'] == [1024, 2048] and line['save_each'] is True
        assert line['train_args']['model'] == 'basic'
        base = os.path.join(out, k + '_leftImg8bit')
        mask = np.load(base + '.npy')
        assert mask.dtype == np.bool_ and mask.shape == (1024, 2048)
        assert np.array_equal(np.load(base + '_scores.npy'), mask)        # the mask again, as the reference writes it
        gt = e2e['labels'][k]
        m = gt >= 0
        conf = np.bincount(2 * gt[m] + mask[m].astype(np.int64), minlength=4).reshape(2, 2)
        assert (line['TP'], line['FP'], line['FN']) == (int(conf[1, 1]), int(conf[0, 1]), int(conf[1, 0]))


def test_save_labels_returns_scores(e2e):
    sys.path.insert(0, ROOT)
    lfs = importlib.import_module('labels_from_segnet')
    out = str(e2e['dir'] / 'out_mem')
    res = lfs.save_labels(e2e['param_dir'], 2000, 0, e2e['img_zip'], e2e['label_zip'], out, 1, 2, False,
                          [1024, 2048], save_each=False, figure=False)
    base = os.path.join(out, e2e['keys'][1] + '_leftImg8bit')
    assert sorted(res) == [base, base + '_scores']
    sc = res[base + '_scores']
    assert sc.dtype == np.float32 and sc.shape == (2, 1024, 2048)
    assert np.array_equal(res[base], np.argmax(sc, 0).astype(bool))
    with pytest.raises(ValueError, match='end_index'):
        lfs.save_labels(e2e['param_dir'], 2000, 0, e2e['img_zip'], e2e['label_zip'], out, 0, 3, False, [1024, 2048])
