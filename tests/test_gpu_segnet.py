"""GPU tests of SegNet-Basic inference (labels_from_segnet.py) on libspalign's kernels: every layer kind against a
float64 restatement of models/segnet_basic.py built from torch CPU ops and Chainer's LRN formula, the Pillow BILINEAR
score resize bit for bit, the whole predict at the training size, determinism across batch sizes, the refusals, and
the labels_from_segnet.py driver end to end on a synthetic zipped dataset."""
import ctypes
import importlib
import io
import json
import os
import subprocess
import sys
import zipfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
F = torch.nn.functional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
segnet = importlib.import_module('superpixel-align_amd.segnet')


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


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


# ------------------------------------------------------------------------------- float64 oracle
def t64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def standardise(x):
    """the dataset's two float32 operations on the 0..255 image"""
    x = np.asarray(x, np.float32).copy()
    x -= segnet.MEAN[None, :, None, None]
    x /= segnet.STD[None, :, None, None]
    return x


def lrn_chainer(x):
    s = (x * x).sum(1, keepdim=True)                 # n = 5 covers all three channels
    return x * (1.0 + 1e-4 / 5 * s) ** -0.75


def conv7(h, w):
    """float64 7x7 convolution, padding 3, in strips of 64 output rows (bounded im2col memory at 512 x 1024)"""
    H = h.shape[2]
    hp = F.pad(h, (0, 0, 3, 3))
    return torch.cat([F.conv2d(hp[:, :, y0:min(y0 + 64, H) + 6], w, padding=(0, 3)) for y0 in range(0, H, 64)], 2)


def bn_conv(p, name, h):
    y = conv7(h, t64(p[name + '/W']))
    g, be, mu, var = (t64(p['%s_bn/%s' % (name, k)])[None, :, None, None] for k in segnet.BN_PARAMS)
    return g * (y - mu) / torch.sqrt(var + segnet.BN_EPS) + be


def windows(h):
    B, C, H, W = h.shape
    return h.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def pool_argmax(h):
    win = windows(h)
    idx = win.argmax(-1)
    return win.gather(-1, idx[..., None])[..., 0], idx


def unpool(h, idx):
    B, C, h2, w2 = h.shape
    out = torch.zeros(B, C, h2, w2, 4, dtype=torch.float64)
    out.scatter_(-1, idx.long()[..., None], h[..., None])
    return out.reshape(B, C, h2, w2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * h2, 2 * w2)


def classify(p, h):
    z = F.conv2d(h, t64(p['conv_classifier/W']), t64(p['conv_classifier/b']))
    return torch.softmax(z, 1)


def forward64(p, img, dev_idx=None):
    """img (B,3,H,W) 0..255 -> float64 probabilities (B,2,H,W).  dev_idx: the device's pooling indices, taken where the
    window's top two oracle values are closer than 1e-5 max|y| (a near-tie either side may resolve differently; an
    unpooled value in the other position of its block is an O(1) change) and required equal everywhere else."""
    h = lrn_chainer(t64(standardise(img)))
    idxs = []
    for li, name in enumerate(segnet.ENCODERS):
        y = torch.relu(bn_conv(p, name, h))
        h, i = pool_argmax(y)
        if dev_idx is not None:
            tol = 1e-5 * float(y.abs().max())
            top2 = windows(y).sort(-1, descending=True).values
            near = (top2[..., 0] - top2[..., 1]) < tol
            d = dev_idx[li].cpu().long()
            assert int(((d != i) & ~near).sum()) == 0, name
            i = torch.where(near, d, i)
            h = windows(y).gather(-1, i[..., None])[..., 0]
        idxs.append(i)
    for name, i in zip(segnet.DECODERS, idxs[::-1]):
        h = bn_conv(p, name, unpool(h, i))
    return classify(p, h)


def dev_weights(p, name, dev='cuda'):
    w, b = segnet.fold_bn(p)[name]
    return torch.from_numpy(segnet.pack_weight(w)).to(dev), torch.from_numpy(b).to(dev)


def nchw64(t):
    return t.detach().cpu().double()


def check_pool(pooled, idx, ref):
    """values within 1e-5 max|y|; indices equal except where the window's top two oracle values are closer than that"""
    yv, yi = pool_argmax(ref)
    tol = 1e-5 * float(ref.abs().max())
    assert float((nchw64(pooled) - yv).abs().max()) <= tol
    top2 = windows(ref).sort(-1, descending=True).values
    near = (top2[..., 0] - top2[..., 1]) < tol
    bad = (idx.cpu().long() != yi) & ~near
    assert int(bad.sum()) == 0, '%d pooling indices differ outside near-ties' % int(bad.sum())
    return yv, yi


# ------------------------------------------------------------------------------- layers
def test_encoder_conv1_lrn(eng):
    p = random_params(10)
    g = np.random.default_rng(11)
    img = g.integers(0, 256, (2, 3, 48, 96)).astype(np.float32)
    w, b = dev_weights(p, 'conv1')
    pooled, idx = eng.segnet_encode(torch.from_numpy(img).cuda(), w, b, segnet.MEAN, segnet.STD)
    torch.cuda.synchronize()
    assert pooled.shape == (2, 64, 24, 48) and pooled.is_contiguous(memory_format=torch.channels_last)
    ref = torch.relu(bn_conv(p, 'conv1', lrn_chainer(t64(standardise(img)))))
    check_pool(pooled, idx, ref)


@pytest.mark.parametrize('H,W', [(32, 64), (20, 36)])
def test_encoder_64(eng, H, W):
    p = random_params(12)
    x = torch.randn((3, 64, H, W), generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    xd = x.float().cuda().contiguous(memory_format=torch.channels_last)
    w, b = dev_weights(p, 'conv2')
    pooled, idx = eng.segnet_encode(xd, w, b)
    torch.cuda.synchronize()
    ref = torch.relu(bn_conv(p, 'conv2', xd.cpu().double()))
    check_pool(pooled, idx, ref)


def test_decoder_on_device_pool(eng):
    p = random_params(14)
    x = torch.randn((2, 64, 32, 64), generator=torch.Generator().manual_seed(15)).cuda().contiguous(
        memory_format=torch.channels_last)
    w2, b2 = dev_weights(p, 'conv3')
    pooled, idx = eng.segnet_encode(x, w2, b2)
    w, b = dev_weights(p, 'conv_decode3')
    y = eng.segnet_decode(pooled, idx, w, b)
    torch.cuda.synchronize()
    assert y.shape == (2, 64, 32, 64) and y.is_contiguous(memory_format=torch.channels_last)
    ref = bn_conv(p, 'conv_decode3', unpool(nchw64(pooled), idx.cpu()))
    assert float((nchw64(y) - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_decode1_classifier_softmax(eng):
    p = random_params(16)
    x = torch.randn((2, 64, 32, 48), generator=torch.Generator().manual_seed(17)).cuda().contiguous(
        memory_format=torch.channels_last)
    we, be = dev_weights(p, 'conv4')
    pooled, idx = eng.segnet_encode(x, we, be)
    w, b = dev_weights(p, 'conv_decode1')
    wc, bc = segnet.fold_bn(p)['conv_classifier']
    prob = eng.segnet_decode(pooled, idx, w, b, torch.from_numpy(wc).cuda(), torch.from_numpy(bc).cuda())
    torch.cuda.synchronize()
    assert prob.shape == (2, 2, 32, 48) and prob.is_contiguous()
    ref = classify(p, bn_conv(p, 'conv_decode1', unpool(nchw64(pooled), idx.cpu())))
    assert float((nchw64(prob) - ref).abs().max()) <= 1e-5


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
    ref = forward64(p, img, [i for _, i in trace]).numpy()
    for bi in range(2):
        label, score = out[bi]
        assert label.shape == (1024, 2048) and score.shape == (2, 1024, 2048) and score.dtype == np.float32
        # the float64 probabilities through the same (host) resize: the remaining difference is the network's rounding
        want = segnet.resize_bilinear_pil(ref[bi].astype(np.float32), (1024, 2048))
        assert float(np.abs(score - want).max()) <= 1e-4
        near = np.abs(want[1] - want[0]) < 1e-3
        assert np.array_equal(label[~near], np.argmax(want, 0)[~near])


def test_determinism_batch_position(eng):
    p = random_params(21)
    model = segnet.SegNetBasic(p, engine=eng)
    g = np.random.default_rng(22)
    imgs = torch.from_numpy(g.integers(0, 256, (3, 3, 64, 128)).astype(np.float32)).cuda()
    one = model.forward(imgs[1:2].contiguous())
    three = model.forward(imgs)
    again = model.forward(imgs)
    torch.cuda.synchronize()
    assert torch.equal(one[0], three[1])
    assert torch.equal(three, again)


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
    pooled = torch.full((1 << 18,), 7.0, device='cuda')
    idx = torch.full((1 << 18,), 9, dtype=torch.uint8, device='cuda')
    m = (ctypes.c_float * 3)(*segnet.MEAN)
    sd = (ctypes.c_float * 3)(*segnet.STD)
    NHWC, NCHW = 0, 1
    cases = [
        # conv1 at H = 40 (not a multiple of 16)
        (lib.spa_segnet_encode(ctx, P(x3), NCHW, 1, 40, 48, 3, P(w3), P(b), m, sd, P(pooled), P(idx), s), -1),
        # a 64-channel stage at an odd width
        (lib.spa_segnet_encode(ctx, P(x64), NHWC, 1, 32, 31, 64, P(w64), P(b), None, None, P(pooled), P(idx), s), -1),
        # Cin 16
        (lib.spa_segnet_encode(ctx, P(x64), NHWC, 1, 32, 32, 16, P(w64), P(b), None, None, P(pooled), P(idx), s), -1),
        # 64 channels stored planar
        (lib.spa_segnet_encode(ctx, P(x64), NCHW, 1, 32, 32, 64, P(w64), P(b), None, None, P(pooled), P(idx), s), -4),
        # conv1 image stored channels-last
        (lib.spa_segnet_encode(ctx, P(x3), NHWC, 1, 48, 48, 3, P(w3), P(b), m, sd, P(pooled), P(idx), s), -4),
        # decoder input stored planar
        (lib.spa_segnet_decode(ctx, P(x64), P(idx), NCHW, 1, 16, 16, P(w64), P(b), None, None, P(pooled), s), -4),
        # decode1 output 2 x (20, 20) = (40, 40): not a multiple of 16
        (lib.spa_segnet_decode(ctx, P(x64), P(idx), NHWC, 1, 20, 20, P(w64), P(b), P(b), P(b), P(pooled), s), -1),
        # score: a downscale
        (lib.spa_segnet_score(ctx, P(x64), 1, 32, 32, 16, 64, P(idx), None, s), -1),
    ]
    torch.cuda.synchronize()
    assert [rc for rc, _ in cases] == [want for _, want in cases]
    assert bool((pooled == 7.0).all()) and bool((idx == 9).all())         # nothing was written
    # the engine wrapper raises on the same shapes
    with pytest.raises(Exception, match='-4'):
        eng.segnet_encode(torch.zeros((1, 64, 32, 32), device='cuda'), w64, b)
    with pytest.raises(Exception, match='-1'):
        eng.segnet_encode(torch.zeros((1, 3, 40, 48), device='cuda'), w3, b, segnet.MEAN, segnet.STD)


# ------------------------------------------------------------------------------- labels_from_segnet.py end to end
def _png(a):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, format='PNG')
    return b.getvalue()


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
            zi.writestr('leftImg8bit/val/%s/%s_leftImg8bit.png' % (city, k), _png(img.astype(np.uint8)))
            lab = np.where(yy > 600, 7, g.integers(0, 12, (1024, 2048))).astype(np.uint8)
            labels[k] = np.where(lab <= 6, -1, np.where(lab == 7, 1, 0))
            zl.writestr('gtFine/val/%s/%s_gtFine_labelIds.png' % (city, k), _png(lab))
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
