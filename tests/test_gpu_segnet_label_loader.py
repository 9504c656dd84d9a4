"""GPU tests of the labelling and validation input stage (labels_from_segnet.py --loader_procs, train_segnet.evaluate's
loader): Engine.segnet_label_eval against segnet_score, confusion and Pillow, bit for bit; its batch-position
determinism and refusals; save_labels and evaluate with the loader against the same calls without it, also where
batches fall back to the host path or a label is refused; the CLI; and what a loader run leaves behind.  Every child
runs under a time limit; a failing child ends the test."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_ref as sref  # noqa: E402
import segnet_train_synth as syn  # noqa: E402

segnet = importlib.import_module('superpixel-align_amd.segnet')
st = importlib.import_module('superpixel-align_amd.segnet_train')
sl = importlib.import_module('superpixel-align_amd.segnet_loader')
lfs = importlib.import_module('labels_from_segnet')
train_segnet = importlib.import_module('train_segnet')

TIMEOUT = 600
# (h, w) -> (H, W): the 2x case; non-integer ratios with W no multiple of 4 or of the block width; equal sizes; one axis
SHAPES = [((32, 48), (64, 96)), ((40, 56), (97, 131)), ((64, 96), (64, 96)), ((16, 32), (16, 83))]


@pytest.fixture(scope='module')
def eng():
    return importlib.import_module('superpixel-align_amd.engine').default_engine()


def _prob(src, B=3, seed=18):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((B, 2) + src, generator=g)
    z[:, :, :4, :4] = 0.0                                           # exact ties: class 0
    return torch.softmax(z, 1).cuda().contiguous()


def _ids(dst, B=3, seed=5):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 34, (B,) + dst).astype(np.uint8)
    ids[:, 3:6] = 255                                               # a band of 255: non-road
    ids[:, 8:11] = rng.integers(0, 7, (B, 3, dst[1]))               # a band that is all ignored
    return ids


def _bincount(mask, ids):
    gt = segnet.label_mask(ids)
    out = np.zeros((len(ids), 4), np.int64)
    for b in range(len(ids)):
        m = gt[b] >= 0
        out[b] = np.bincount(2 * gt[b][m] + mask[b][m].astype(np.int64), minlength=4)
    return out


# ------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('want_scores', [False, True])
@pytest.mark.parametrize('src,dst', SHAPES)
def test_label_eval_equals_score_confusion_and_pillow(eng, src, dst, want_scores):
    from PIL import Image
    prob = _prob(src)
    ids = _ids(dst)
    ids[2] = np.random.default_rng(6).integers(0, 7, dst)          # an image of ignored ids only
    mask0, sc0 = eng.segnet_score(prob, dst, want_scores=True)
    mask, sc, counts = eng.segnet_label_eval(prob, dst, torch.from_numpy(ids).cuda(), want_scores=want_scores)
    conf = eng.confusion(mask0, torch.from_numpy(segnet.label_mask(ids)).cuda())
    torch.cuda.synchronize()
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (3,) + dst
    assert np.array_equal(mask.cpu().numpy(), mask0.cpu().numpy())
    if want_scores:
        assert sc.dtype == torch.float32 and tuple(sc.shape) == (3, 2) + dst
        assert np.array_equal(syn.bits(sc.cpu().numpy()), syn.bits(sc0.cpu().numpy()))
        ph = prob.cpu().numpy()
        for bi in range(3):
            want = np.stack([np.asarray(Image.fromarray(c, mode='F').resize(dst[::-1], Image.BILINEAR), np.float32)
                             for c in ph[bi]])
            assert np.array_equal(syn.bits(sc[bi].cpu().numpy()), syn.bits(want))
    else:
        assert sc is None
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (3, 4)
    assert np.array_equal(counts.cpu().numpy(), conf.cpu().numpy())
    assert np.array_equal(counts.cpu().numpy(), _bincount(mask0.cpu().numpy(), ids))
    assert counts[2].tolist() == [0, 0, 0, 0] and int(counts[:2].sum()) > 0
    # without labels: the mask and the scores only
    mask1, sc1, none = eng.segnet_label_eval(prob, dst, None, want_scores=want_scores)
    assert none is None and torch.equal(mask1, mask0) and (sc1 is None) == (not want_scores)
    if want_scores:
        assert np.array_equal(syn.bits(sc1.cpu().numpy()), syn.bits(sc0.cpu().numpy()))


def test_label_eval_batch_position(eng):
    src, dst = (40, 56), (97, 131)
    one = _prob(src, B=1, seed=3)
    other = _prob(src, B=2, seed=4)
    prob = torch.cat([one, other[:1], one]).contiguous()
    i1, i2 = _ids(dst, B=1, seed=7), _ids(dst, B=1, seed=8)
    ids = torch.from_numpy(np.concatenate([i1, i2, i1])).cuda()
    a = eng.segnet_label_eval(one, dst, ids[:1].contiguous(), want_scores=True)
    b = eng.segnet_label_eval(prob, dst, ids, want_scores=True)
    c = eng.segnet_label_eval(prob, dst, ids, want_scores=True)
    torch.cuda.synchronize()
    for pos in (0, 2):
        assert torch.equal(a[0][0], b[0][pos]) and torch.equal(a[2][0], b[2][pos])
        assert np.array_equal(syn.bits(a[1][0].cpu().numpy()), syn.bits(b[1][pos].cpu().numpy()))
    assert torch.equal(b[0], c[0]) and torch.equal(b[2], c[2])
    assert np.array_equal(syn.bits(b[1].cpu().numpy()), syn.bits(c[1].cpu().numpy()))


def test_label_eval_refusals_launch_nothing(eng):
    lib, ctx = eng._lib, eng._ctx
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    prob = _prob((32, 32), B=1)
    ids = torch.full((1, 64, 64), 7, dtype=torch.uint8, device='cuda')
    mask = torch.full((1 << 14,), 9, dtype=torch.uint8, device='cuda')
    sc = torch.full((1 << 15,), 7.0, device='cuda')
    counts = torch.full((4,), -5, dtype=torch.int64, device='cuda')
    # a downscale
    assert lib.spa_segnet_label_eval(ctx, P(prob), 1, 32, 32, 16, 64, P(ids), P(mask), P(sc), P(counts), s) == -1
    assert 'downscale' in lib.spa_last_error().decode()
    # labels without counts, counts without labels
    assert lib.spa_segnet_label_eval(ctx, P(prob), 1, 32, 32, 64, 64, P(ids), P(mask), P(sc), None, s) == -1
    assert 'label_ids and counts' in lib.spa_last_error().decode()
    assert lib.spa_segnet_label_eval(ctx, P(prob), 1, 32, 32, 64, 64, None, P(mask), P(sc), P(counts), s) == -1
    assert 'label_ids and counts' in lib.spa_last_error().decode()
    # a non-positive size
    assert lib.spa_segnet_label_eval(ctx, P(prob), 1, 32, 32, 0, 64, P(ids), P(mask), P(sc), P(counts), s) == -1
    assert 'H > 0' in lib.spa_last_error().decode()
    # the wrapper: a label whose shape is not (H, W), and the downscale
    with pytest.raises(Exception, match='label_ids'):
        eng.segnet_label_eval(prob, (64, 64), ids[:, :48].contiguous())
    with pytest.raises(Exception, match='-1'):
        eng.segnet_label_eval(prob, (16, 64))
    torch.cuda.synchronize()
    assert bool((mask == 9).all()) and bool((sc == 7.0).all()) and bool((counts == -5).all())


# ------------------------------------------------------------------------------- save_labels
H, W = 64, 96
IN_SHAPE = (32, 48)


@pytest.fixture(scope='module')
def labset(tmp_path_factory):
    d = tmp_path_factory.mktemp('label_loader')
    z = syn.write(str(d / 'data'), 0, 5, H, W)
    param_dir = d / 'run'
    param_dir.mkdir()
    with open(str(param_dir / 'args.txt'), 'w') as f:
        json.dump({'model': 'basic', 'input_shape': list(IN_SHAPE), 'batchsize': 2}, f)
    with open(str(param_dir / 'snapshot_iter_7'), 'wb') as f:
        np.savez(f, **{segnet.PREFIX + k: v for k, v in sref.random_params(24).items()})
    rng = np.random.default_rng(2)
    # the fall-back set: frame 2 stored larger (its label is not), frame 4 as a grey PNG
    fb_imgs = syn.rewrite(z[2], str(d / 'fb_imgs.zip'),
                          {2: lambda b: syn.png(rng.integers(0, 256, (80, 112, 3), dtype=np.uint8)),
                           4: lambda b: syn.png(syn.decoded(b)[:, :, 1].copy())})
    bad_labs = syn.rewrite(z[3], str(d / 'bad_labs.zip'), {3: lambda b: syn.png(syn.decoded(b)[:48].copy())})
    return dict(dir=d, imgs=z[2], labs=z[3], fb_imgs=fb_imgs, bad_labs=bad_labs, param_dir=str(param_dir))


def _save(labset, out, procs, imgs=None, labs=None, save_each=True, stats=None, on_labels=None, **kw):
    return lfs.save_labels(labset['param_dir'], 7, 0, imgs or labset['imgs'], labs or labset['labs'], out, 0, 5, False,
                           [H, W], save_each=save_each, figure=False, batchsize=2, loader_procs=procs,
                           loader_stats=stats, on_labels=on_labels, **kw)


def _files(out):
    return {f: open(os.path.join(out, f), 'rb').read() for f in sorted(os.listdir(out)) if f.endswith('.npy')}


def _lines(out):
    lines = [json.loads(l) for l in open(os.path.join(out, 'result.json'))]
    for l in lines:
        assert l.pop('out_dir') == out
    return lines


def _same_arrays(a, b):
    assert [os.path.basename(k) for k in a] == [os.path.basename(k) for k in b]
    for (ka, va), (kb, vb) in zip(a.items(), b.items()):
        assert va.dtype == vb.dtype and va.shape == vb.shape and va.flags.owndata and vb.flags.owndata, ka
        assert np.array_equal(syn.bits(va), syn.bits(vb)), ka


def _workers_gone(stats, shm_before):
    import multiprocessing
    for pid in stats['worker_pids']:
        try:
            with open('/proc/%d/stat' % pid) as f:
                assert f.read().rsplit(')', 1)[1].split()[0] == 'Z', pid
        except OSError:
            pass
    assert [p for p in multiprocessing.active_children() if p.pid in stats['worker_pids']] == []
    assert syn.shm_names('psm_') == shm_before


@pytest.mark.parametrize('split', [False, True])
def test_save_labels_with_the_loader_equals_the_plain_loop(labset, tmp_path, split):
    kw = {'split_planes': True} if split else {}
    shm_before = syn.shm_names('psm_')
    plain, loaded = str(tmp_path / 'plain'), str(tmp_path / 'loaded')
    stats = {}
    _save(labset, plain, 0, **kw)
    _save(labset, loaded, 2, stats=stats, **kw)
    fa, fb = _files(plain), _files(loaded)
    assert len(fa) == 10 and fa == fb
    la, lb = _lines(plain), _lines(loaded)
    assert len(la) == 5 and la == lb and [l['img_fn'] for l in la] == sorted(l['img_fn'] for l in la)
    assert all(l.get('split_planes', False) is split for l in lb) and any(l['TP'] + l['FP'] + l['FN'] > 0 for l in la)
    assert stats['n_host_batches'] == 0 and 1 <= len(stats['worker_pids']) <= 2 and stats['pinned'] in (True, False)
    _workers_gone(stats, shm_before)
    # save_each=False: the returned arrays, then the on_labels sequence (kept without copying: they own their memory)
    ra = _save(labset, plain, 0, save_each=False, **kw)
    rb = _save(labset, loaded, 2, save_each=False, **kw)
    assert len(ra) == 10
    _same_arrays(ra, rb)
    assert rb[sorted(rb)[1]].shape == (2, H, W) and rb[sorted(rb)[0]].dtype == np.bool_
    sa, sb = [], []
    assert _save(labset, plain, 0, save_each=False, on_labels=lambda k, v: sa.append((k, v)), **kw) == {}
    assert _save(labset, loaded, 2, save_each=False, on_labels=lambda k, v: sb.append((k, v)), **kw) == {}
    assert len(sa) == 10 and [os.path.basename(k) for k, _ in sa] == [os.path.basename(k) for k in ra]
    _same_arrays(dict(sa), dict(sb))
    _same_arrays(dict(sb), rb)


def test_save_labels_bf16_with_the_loader_completes(labset, tmp_path):
    out = str(tmp_path / 'bf16')
    stats = {}
    _save(labset, out, 2, stats=stats, dtype='bf16')
    lines = _lines(out)
    assert len(lines) == 5 and all(l['dtype'] == 'bf16' for l in lines) and stats['n_host_batches'] == 0
    for l in lines:
        base = os.path.splitext(os.path.basename(l['img_fn']))[0]
        m = np.load(os.path.join(out, base + '.npy'))
        assert m.dtype == np.bool_ and m.shape == (H, W)


def test_fallback_batches_and_a_refused_label(labset, tmp_path):
    shm_before = syn.shm_names('psm_')
    plain, loaded = str(tmp_path / 'plain'), str(tmp_path / 'loaded')
    stats = {}
    _save(labset, plain, 0, imgs=labset['fb_imgs'])
    _save(labset, loaded, 2, imgs=labset['fb_imgs'], stats=stats)
    assert _files(plain) == _files(loaded) and len(_files(plain)) == 10
    assert _lines(plain) == _lines(loaded)
    assert stats['n_host_batches'] == 2                             # [2, 3] and [4] of [0, 1], [2, 3], [4]
    ra = _save(labset, plain, 0, imgs=labset['fb_imgs'], save_each=False)
    rb = _save(labset, loaded, 2, imgs=labset['fb_imgs'], save_each=False)
    _same_arrays(ra, rb)
    # label 3 is 48 x 96: the same error at the same image, after the same files
    plain, loaded = str(tmp_path / 'plain_bad'), str(tmp_path / 'loaded_bad')
    errs = []
    for out, procs in ((plain, 0), (loaded, 2)):
        stats = {}
        with pytest.raises(ValueError, match='has shape') as e:
            _save(labset, out, procs, labs=labset['bad_labs'], stats=stats)
        errs.append(str(e.value))
        if procs:
            _workers_gone(stats, shm_before)                        # nothing is left after a run that raises
    assert errs[0] == errs[1] and '(48, 96)' in errs[0]
    assert _files(plain) == _files(loaded) and len(_files(plain)) == 6
    assert _lines(plain) == _lines(loaded) and len(_lines(plain)) == 3


# ------------------------------------------------------------------------------- validation
@pytest.fixture(scope='module')
def trainer(eng):
    tr = st.SegNetTrainer(st.init_params(5), st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy,
                          engine=eng)
    g = torch.Generator().manual_seed(6)
    img = torch.rand((2, 3) + IN_SHAPE, generator=g) * 255
    t = torch.randint(-1, 2, (2,) + IN_SHAPE, generator=g)
    tr.step(img.cuda(), t.cuda())                                   # the running statistics are not the initial ones
    return tr


def _same_report(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k] == b[k] or (isinstance(a[k], float) and np.isnan(a[k]) and np.isnan(b[k])), k


@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('batch', [1, 2])
def test_evaluate_with_the_loader_equals_evaluate_without(labset, trainer, eng, batch, split):
    valid = segnet.ZippedCityscapesRoadDataset(labset['imgs'], labset['labs'], IN_SHAPE)
    want = train_segnet.evaluate(trainer, valid, [H, W], batch, None, split_planes=split)
    loader = sl.LabelLoader(valid, range(5), batch, 2, sl.DeviceLabelStage(eng))
    try:
        got = train_segnet.evaluate(trainer, valid, [H, W], batch, None, split_planes=split, loader=loader)
        again = train_segnet.evaluate(trainer, valid, [H, W], batch, None, split_planes=split, loader=loader)
        assert loader.n_host_batches == 0
    finally:
        loader.close()
    _same_report(want, got)
    _same_report(want, again)
    assert want['val_/main/FP'] + want['val_/main/FN'] > 0


def test_evaluate_fallback_batches(labset, trainer, eng):
    valid = segnet.ZippedCityscapesRoadDataset(labset['fb_imgs'], labset['labs'], IN_SHAPE)
    want = train_segnet.evaluate(trainer, valid, [H, W], 2, [1, 2, 3, 4])
    loader = sl.LabelLoader(valid, [1, 2, 3, 4], 2, 2, sl.DeviceLabelStage(eng))
    try:
        got = train_segnet.evaluate(trainer, valid, [H, W], 2, [1, 2, 3, 4], loader=loader)
        assert loader.n_host_batches == 2                           # [1, 2] and [3, 4] both hold an odd frame
        with pytest.raises(ValueError, match='other indices'):
            train_segnet.evaluate(trainer, valid, [H, W], 2, [0, 1], loader=loader)
    finally:
        loader.close()
    _same_report(want, got)


# ------------------------------------------------------------------------------- the CLI
def test_cli_with_the_loader(labset, tmp_path):
    plain, out = str(tmp_path / 'plain'), str(tmp_path / 'cli')
    _save(labset, plain, 0)
    cmd = [sys.executable, os.path.join(ROOT, 'labels_from_segnet.py'), '--param_dir', labset['param_dir'],
           '--iteration', '7', '--gpu', '0', '--img_zip_fn', labset['imgs'], '--label_zip_fn', labset['labs'],
           '--out_dir', out, '--start_index', '0', '--end_index', '5', '--eval_shape', str(H), str(W), '--no_figure',
           '--batchsize', '2', '--loader_procs', '2']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'decoded on the host' not in r.stdout
    assert _files(out) == _files(plain) and len(_files(out)) == 10
    assert _lines(out) == _lines(plain)
