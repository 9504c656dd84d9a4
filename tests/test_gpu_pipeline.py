"""GPU tests of the layers above the kernels: the DRN module on the device, the five drop-in
ops (reference signatures, host arrays), the fused LabelPipeline and the two CLI drivers —
each compared with the CPU oracle on the same inputs."""
import importlib
import json
import os
import sys
import types
import zlib

import numpy as np
import pytest

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def _args(**kw):
    d = dict(superpixel_method='slic', n_slic_segments=40, n_anchors=10, n_neighbors=4,
             without_pos=False, y_rel_pos=0.75, x_rel_pos=0.5, y_rel_sigma=0.1, x_rel_sigma=0.1,
             gpu=0, n_clusters=2, use_feature_maps=[7], pool_mode='anchor', mean_sampling='nearest',
             arch='drn_d_22', dtype='fp32', drn_weights=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.fixture(scope='module')
def mods():
    names = ('ops', 'pipeline', 'drn', 'cli', 'engine')
    return types.SimpleNamespace(**{n: importlib.import_module('superpixel-align_amd.' + n) for n in names})


def test_drn_on_gpu_matches_reference_maps(mods):
    from test_host_cpu import det_fill
    g = golden('drn_maps')
    for name in ('drn_c_26', 'drn_d_22'):
        m = mods.drn.DRN(name)
        det_fill(m)
        m.prepare('cuda', torch.float32, fold_bn=True)
        _, maps = m.batch_predict(g['x'])
        got = maps[7].float().cpu().numpy()
        assert maps[7].is_contiguous(memory_format=torch.channels_last)
        scale = float(np.abs(g[name + '_map7']).max())
        np.testing.assert_allclose(got, g[name + '_map7'], rtol=1e-4, atol=1e-4 * scale)   # north star: 1e-4
        mb = mods.drn.DRN(name)
        det_fill(mb)
        mb.prepare('cuda', torch.bfloat16, fold_bn=True)
        _, mapsb = mb.batch_predict(g['x'])
        assert mapsb[7].dtype == torch.bfloat16
        err = np.abs(mapsb[7].float().cpu().numpy() - g[name + '_map7']).max() / scale
        assert err < 0.05, err                     # bf16 storage + fp32 accumulation


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_drn_streams_two_equals_one(mods, synth, dtype):
    """DRN.batch_predict(streams=2): both halves run the fused stem concurrently on side streams with ONE context;
    every call owns its normalised-image scratch, so the maps equal those of the same two halves run one after the
    other on one stream (same shapes, hence the same MIOpen solvers) bit for bit — the bf16 stem used to share the
    context-wide workspace between the streams."""
    td = {'bf16': torch.bfloat16, 'fp32': torch.float32}[dtype]
    m = mods.drn.create_drn('drn_d_22', device='cuda', dtype=td)
    x = synth.synth_batch(list(range(40, 48)), 256, 512)
    for _ in range(3):
        _, one = m.batch_predict(x, sub_batch=4, need=[1, 7], streams=1)
        _, two = m.batch_predict(x, need=[1, 7], streams=2)
        torch.cuda.synchronize()
        for i in (1, 7):
            if dtype == 'bf16':
                assert torch.equal(one[i], two[i]), i
            else:
                # float32: MIOpen's solver for a layer may accumulate through atomics (split-K), so two runs of the
                # same shapes agree to rounding only; a stem race would show as O(1) differences
                scale = float(one[i].abs().max())
                assert float((one[i] - two[i]).abs().max()) <= 2e-5 * scale, i


def test_five_ops_drop_in(mods, orc, synth):
    """The reference call sequence (utils/apply_spalign_kmeans.py:30-57) with host arrays."""
    ops = mods.ops
    args = _args()
    H, W, B = 128, 256, 2
    imgs = synth.synth_batch([21, 22], H, W)
    keep = imgs.copy()
    fmaps = synth.synth_feature_map(5, 32, H // 8, W // 8, batch=B)
    ops.seed(1111)
    sps = ops.batch_superpixel(args, imgs)
    assert sps.dtype == np.int64 and sps.shape == (B, H, W) and np.array_equal(imgs, keep)
    ref_sps = orc.batch_superpixel(args, imgs)
    assert np.array_equal(sps, ref_sps)
    model = types.SimpleNamespace(xp=np)
    feats, n_per = ops.batch_superpixel_align(args, model, imgs, sps, fmaps)
    rf, rn = orc.batch_superpixel_align(args, imgs, ref_sps, fmaps, orc.PyRandom(1111))
    assert n_per == rn and feats.dtype == np.float64 and np.array_equal(feats, rf)
    w = ops.batch_create_prior(args, sps)
    np.testing.assert_allclose(w, orc.batch_create_prior(args, ref_sps), rtol=1e-12)
    cl, road = ops.batch_weighted_kmeans(args, sps, feats, w, n_per)
    rcl, rroad, _ = orc.batch_weighted_kmeans(args, ref_sps, rf, orc.batch_create_prior(args, ref_sps), rn)
    assert cl.dtype == np.int64 and road.dtype == np.bool_
    assert np.array_equal(cl, rcl) and np.array_equal(road, rroad)
    # fresh host arrays (no device cache hit) take the upload path and give the same answer
    cl2, road2 = ops.batch_weighted_kmeans(args, sps.copy(), feats.copy(), w.copy(), list(n_per))
    assert np.array_equal(cl2, cl)
    # k = 4 goes through numpy's global shuffle stream
    a4 = _args(n_clusters=4)
    ops.seed(1111)
    cl4, _ = ops.batch_weighted_kmeans(a4, sps, feats, w, n_per)
    r4, _, _ = orc.batch_weighted_kmeans(a4, ref_sps, rf, w, rn, nprandom=orc.NpRandom(1111))
    assert np.array_equal(cl4, r4)
    # the felzenszwalb branch (the reference launchers' choice) through the same boundary
    af = _args(superpixel_method='felzenszwalb', felzenszwalb_scale=300.0, felzenszwalb_sigma=0.8,
               felzenszwalb_min_size=20)
    scenes = np.stack([synth.synth_scene(s, 96, 160) for s in (50, 51)])
    fz = ops.batch_superpixel(af, scenes)
    assert fz.dtype == np.int64 and np.array_equal(fz, orc.batch_superpixel(af, scenes))


@pytest.mark.parametrize('pool_mode,k', [('mean', 2), ('anchor', 2), ('anchor', 4), ('mean', 3), ('anchor_dev', 2)])
def test_fused_pipeline_end_to_end(mods, orc, synth, pool_mode, k):
    device_rng = pool_mode == 'anchor_dev'           # anchors drawn on the device (spa_anchor_ranks_dev)
    pool_mode = 'anchor' if device_rng else pool_mode
    args = _args(pool_mode=pool_mode, n_clusters=k, n_slic_segments=60, device_rng=device_rng)
    H, W, B = 160, 320, 3
    imgs = synth.synth_batch([31, 32, 33], H, W)
    model = mods.drn.create_drn('drn_d_22', device='cuda')
    pipe = mods.pipeline.LabelPipeline(args, model, mods.ops.engine())
    res = pipe.run(imgs)
    t = pipe.elapsed_times()
    assert set(t) >= {'time_superpixel', 'time_roialign', 'time_prior', 'time_kmeans', 'time_feature_maps'}
    fmap = res.fmap.float().cpu().numpy()
    sps = np.stack([orc.slic(im, 60) for im in imgs])
    assert np.array_equal(res.labels.cpu().numpy().astype(np.int64), sps)
    feats, n_per = orc.batch_superpixel_align(args, imgs, sps, fmap, orc.PyRandom(1111), pool_mode)
    N = sum(n_per)
    assert res.n_labels.cpu().tolist() == n_per
    assert np.array_equal(res.X[:N].cpu().numpy(), feats)
    prior = orc.batch_create_prior(args, sps)
    np.testing.assert_allclose(res.prior[:N].cpu().numpy(), prior, rtol=1e-12)
    cl, road, info = orc.batch_weighted_kmeans(args, sps, feats, prior, n_per, nprandom=orc.NpRandom(1111))
    gi = res.info.cpu().tolist()
    assert gi[:3] == [info['n_iter'], info['status'], N]
    assert np.array_equal(res.assign[:N].cpu().numpy(), info['assign'])
    assert np.array_equal(res.cluster.cpu().numpy(), cl)
    assert np.array_equal(res.road.cpu().numpy().astype(bool), road)


def test_reference_operating_point_felzenszwalb(mods, orc, synth):
    """What every reference launcher runs (utils/create_random300_labels.sh:14-34): 224x224 input,
    felzenszwalb(scale 300, sigma 0.8, min_size 20), DRN-C-26 layer8, 10 anchors, k = 4, batch."""
    args = _args(superpixel_method='felzenszwalb', felzenszwalb_scale=300.0, felzenszwalb_sigma=0.8,
                 felzenszwalb_min_size=20, n_clusters=4, pool_mode='anchor', arch='drn_c_26')
    imgs = np.stack([synth.synth_scene(60 + i, 224, 224) for i in range(6)])
    model = mods.drn.create_drn('drn_c_26', device='cuda')
    pipe = mods.pipeline.LabelPipeline(args, model, mods.ops.engine())
    res = pipe.run(imgs)
    fmap = res.fmap.float().cpu().numpy()
    sps = orc.batch_superpixel(args, imgs)
    assert np.array_equal(res.labels.cpu().numpy().astype(np.int64), sps)
    feats, n_per = orc.batch_superpixel_align(args, imgs, sps, fmap, orc.PyRandom(1111), 'anchor')
    N = sum(n_per)
    assert np.array_equal(res.X[:N].cpu().numpy(), feats)
    prior = orc.batch_create_prior(args, sps)
    np.testing.assert_allclose(res.prior[:N].cpu().numpy(), prior, rtol=1e-12)
    cl, road, info = orc.batch_weighted_kmeans(args, sps, feats, prior, n_per, nprandom=orc.NpRandom(1111))
    assert np.array_equal(res.cluster.cpu().numpy(), cl)
    assert np.array_equal(res.road.cpu().numpy().astype(bool), road)


def test_cli_drivers_on_synthetic_pngs(mods, orc, synth, tmp_path):
    from PIL import Image
    H, W, n = 96, 192, 5
    img_fns, lab_fns = [], []
    for i in range(n):
        img = synth.synth_image(40 + i, H, W, integer_valued=True).astype(np.uint8)
        fn = str(tmp_path / ('city_%06d_000019_leftImg8bit.png' % i))
        Image.fromarray(img.transpose(1, 2, 0)).save(fn)
        lf = str(tmp_path / ('city_%06d_000019_gtFine_labelIds.png' % i))
        Image.fromarray(synth.synth_gt_labels(40 + i, 2 * H, 2 * W)).save(lf)    # GT at another size
        img_fns.append(fn); lab_fns.append(lf)
    (tmp_path / 'imgs.txt').write_text('\n'.join(img_fns) + '\n')
    (tmp_path / 'labs.txt').write_text('\n'.join(lab_fns) + '\n')
    out = tmp_path / 'out'
    argv = ['--superpixel_method', 'slic', '--n_slic_segments', '30', '--n_clusters', '2',
            '--resize_shape', str(H), str(W), '--batchsize', '2', '--out_dir', str(out),
            '--img_file_list', str(tmp_path / 'imgs.txt'), '--label_file_list', str(tmp_path / 'labs.txt'),
            '--start_index', '0', '--end_index', str(n), '--arch', 'drn_d_22', '--pool_mode', 'mean', '--no_figure']
    assert mods.cli.main_labelled(argv) == 0
    lines = [json.loads(l) for l in open(out / 'result.json')]
    assert len(lines) == 6                                   # batches (0,2) (2,4) (3,5): image 3 twice
    assert [os.path.basename(l['img_fn'])[5:11] for l in lines] == ['000000', '000001', '000002', '000003', '000003', '000004']
    last = {l['img_fn']: l for l in lines}                  # a re-labelled image overwrites its .npy (:539-542)
    for l in last.values():
        base = os.path.splitext(os.path.basename(l['img_fn']))[0]
        road = np.load(out / (base + '.npy'))
        allc = np.load(out / (base + '_all_cluster.npy'))
        assert road.dtype == np.uint8 and road.shape == (2 * H, 2 * W) and set(np.unique(road)) <= {0, 1}
        assert np.array_equal(road, (allc == 0).astype(np.uint8))
        gt = orc.create_label_mask(np.asarray(Image.open(l['label_fn'])))
        sc = orc.confusion(road, gt)
        assert (l['TP'], l['FP'], l['FN']) == (sc['TP'], sc['FP'], sc['FN'])
        assert l['n_clusters'] == 2 and 'time_kmeans' in l and 'elapsed_time' in l
    # label-free driver
    out2 = tmp_path / 'out2'
    argv2 = ['--img_list_fn', str(tmp_path / 'imgs.txt'), '--label_shape', str(2 * H), str(2 * W),
             '--gpu', '0', '--out_dir', str(out2), '--superpixel_method', 'slic', '--n_slic_segments', '30',
             '--n_clusters', '2', '--resize_shape', str(H), str(W), '--batchsize', '5',
             '--start_index', '0', '--end_index', str(n), '--arch', 'drn_d_22', '--pool_mode', 'mean']
    assert mods.cli.main_labelfree(argv2) == 0
    for fn in img_fns:
        m = np.asarray(Image.open(out2 / os.path.basename(fn)))
        assert m.shape == (2 * H, 2 * W) and set(np.unique(m)) <= {0, 1}


def test_driver_sixty_images_every_line_scored_like_the_oracle(mods, orc, synth, tmp_path):
    """README.md:99-107 / batch_spalign_kmeans.py:538-548 at the reference's batch size: 60 PNGs, --batchsize 30,
    run through the root-level script as a child process (the way create_*_labels.sh starts it), then
    utils/mean_result.py.  Every result.json line carries the confusion the oracle computes from the saved .npy
    mask and the decoded ground truth, the batch loop produced each image exactly once, the summary's pooled
    precision / recall follow from the summed counts."""
    import subprocess
    from PIL import Image
    H, W, n = 128, 256, 60
    img_fns, lab_fns = [], []
    for i in range(n):
        img = synth.synth_image(300 + i, H, W, integer_valued=True).astype(np.uint8)
        fn = str(tmp_path / ('burg_%06d_000019_leftImg8bit.png' % i))
        Image.fromarray(img.transpose(1, 2, 0)).save(fn)
        lf = str(tmp_path / ('burg_%06d_000019_gtFine_labelIds.png' % i))
        Image.fromarray(synth.synth_gt_labels(300 + i, H, W)).save(lf)
        img_fns.append(fn); lab_fns.append(lf)
    (tmp_path / 'imgs.txt').write_text('\n'.join(img_fns) + '\n')
    (tmp_path / 'labs.txt').write_text('\n'.join(lab_fns) + '\n')
    out = tmp_path / 'out'
    cmd = [sys.executable, os.path.join(ROOT, 'batch_spalign_kmeans.py'), '--superpixel_method', 'slic',
           '--n_slic_segments', '40', '--n_clusters', '2', '--resize_shape', str(H), str(W), '--batchsize', '30',
           '--out_dir', str(out), '--img_file_list', str(tmp_path / 'imgs.txt'),
           '--label_file_list', str(tmp_path / 'labs.txt'), '--start_index', '0', '--end_index', str(n),
           '--arch', 'drn_d_22', '--pool_mode', 'mean', '--no_figure']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in open(out / 'result.json')]
    assert [l['img_fn'] for l in lines] == img_fns                   # two full batches, index order, no repeats
    tp = fp = fn_ = 0
    for l in lines:
        base = os.path.splitext(os.path.basename(l['img_fn']))[0]
        road = np.load(out / (base + '.npy'))
        allc = np.load(out / (base + '_all_cluster.npy'))
        assert np.array_equal(road, (allc == 0).astype(np.uint8))
        sc = orc.confusion(road, orc.create_label_mask(np.asarray(Image.open(l['label_fn']))))
        assert (l['TP'], l['FP'], l['FN']) == (sc['TP'], sc['FP'], sc['FN'])
        assert l['road_iou'] == sc['road_iou'] and l['batchsize'] == 30 and l['n_slic_segments'] == 40
        tp, fp, fn_ = tp + sc['TP'], fp + sc['FP'], fn_ + sc['FN']
    m = subprocess.run([sys.executable, os.path.join(ROOT, 'utils', 'mean_result.py'), str(out / 'result.json')],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert m.returncode == 0, m.stderr[-1000:]
    txt = open(out / 'summary.txt').read()
    assert ('Precision\t:%s' % (tp / (tp + fp))) in txt and ('Recall\t:%s' % (tp / (tp + fn_))) in txt


def test_driver_gpu_input_stage_equals_host_resize(mods, synth, tmp_path):
    """The labelled driver with the GPU input stage (decode on threads, spa_resize_bicubic_u8) writes the
    same masks and scores as with --host_resize (Pillow on the host threads), images resized 96x192 -> 64x80."""
    from PIL import Image
    H, W, n = 96, 192, 4
    img_fns, lab_fns = [], []
    for i in range(n):
        img = synth.synth_image(80 + i, H, W, integer_valued=True).astype(np.uint8)
        fn = str(tmp_path / ('town_%06d_000019_leftImg8bit.png' % i))
        Image.fromarray(img.transpose(1, 2, 0)).save(fn)
        lf = str(tmp_path / ('town_%06d_000019_gtFine_labelIds.png' % i))
        Image.fromarray(synth.synth_gt_labels(80 + i, H, W)).save(lf)
        img_fns.append(fn); lab_fns.append(lf)
    (tmp_path / 'imgs.txt').write_text('\n'.join(img_fns) + '\n')
    (tmp_path / 'labs.txt').write_text('\n'.join(lab_fns) + '\n')
    outs = []
    # ... and the same for the OpenCV branch of the resize (--resize_backend cv2): device kernel vs the host form
    for extra in ([], ['--host_resize'], ['--resize_backend', 'cv2'], ['--resize_backend', 'cv2', '--host_resize']):
        out = tmp_path / ('out' + str(len(outs)))
        argv = ['--superpixel_method', 'slic', '--n_slic_segments', '20', '--n_clusters', '2',
                '--resize_shape', '64', '80', '--batchsize', '2', '--out_dir', str(out),
                '--img_file_list', str(tmp_path / 'imgs.txt'), '--label_file_list', str(tmp_path / 'labs.txt'),
                '--arch', 'drn_d_22', '--pool_mode', 'mean', '--no_figure'] + extra
        try:
            assert mods.cli.main_labelled(argv) == 0
        finally:
            mods.cli.RESIZE_BACKEND[0] = 'pil'
        outs.append(out)
    for p, q in ((0, 1), (2, 3)):
        for fn in img_fns:
            base = os.path.splitext(os.path.basename(fn))[0]
            for suffix in ('.npy', '_all_cluster.npy'):
                assert np.array_equal(np.load(outs[p] / (base + suffix)), np.load(outs[q] / (base + suffix))), base
        a = [json.loads(l) for l in open(outs[p] / 'result.json')]
        b = [json.loads(l) for l in open(outs[q] / 'result.json')]
        assert [(x['TP'], x['FP'], x['FN']) for x in a] == [(x['TP'], x['FP'], x['FN']) for x in b]


def test_driver_process_decode_equals_thread_decode(mods, synth, tmp_path):
    """--decode_procs N: PNGs decoded by worker processes into pinned shared-memory slabs (decode_worker.py) give the
    same masks and result lines as the thread pool; a batch with a frame of another size falls back to the threads."""
    from PIL import Image
    H, W, n = 96, 192, 7
    img_fns, lab_fns = [], []
    for i in range(n):
        h, w = (80, 100) if i == 5 else (H, W)
        img = synth.synth_image(120 + i, h, w, integer_valued=True).astype(np.uint8)
        fn = str(tmp_path / ('proc_%06d_000019_leftImg8bit.png' % i))
        Image.fromarray(img.transpose(1, 2, 0)).save(fn)
        lf = str(tmp_path / ('proc_%06d_000019_gtFine_labelIds.png' % i))
        Image.fromarray(synth.synth_gt_labels(120 + i, H, W)).save(lf)
        img_fns.append(fn); lab_fns.append(lf)
    (tmp_path / 'imgs.txt').write_text('\n'.join(img_fns) + '\n')
    (tmp_path / 'labs.txt').write_text('\n'.join(lab_fns) + '\n')
    outs = []
    for extra in (['--decode_procs', '3'], []):
        out = tmp_path / ('out' + str(len(outs)))
        argv = ['--superpixel_method', 'slic', '--n_slic_segments', '20', '--n_clusters', '2',
                '--resize_shape', '64', '80', '--batchsize', '2', '--out_dir', str(out),
                '--img_file_list', str(tmp_path / 'imgs.txt'), '--label_file_list', str(tmp_path / 'labs.txt'),
                '--arch', 'drn_d_22', '--pool_mode', 'mean', '--no_figure'] + extra
        assert mods.cli.main_labelled(argv) == 0
        outs.append(out)
    for fn in img_fns:
        base = os.path.splitext(os.path.basename(fn))[0]
        assert np.array_equal(np.load(outs[0] / (base + '.npy')), np.load(outs[1] / (base + '.npy'))), base
    a = [json.loads(l) for l in open(outs[0] / 'result.json')]
    b = [json.loads(l) for l in open(outs[1] / 'result.json')]
    assert [(x['img_fn'], x['TP'], x['FP'], x['FN']) for x in a] == [(x['img_fn'], x['TP'], x['FP'], x['FN']) for x in b]


def test_driver_mixed_size_batch_takes_the_host_path(mods, synth, tmp_path):
    """A batch whose source PNGs differ in size (one of them RGBA) cannot be uploaded as one 8-bit tensor: the
    input stage falls back to the host resize on the frames it already decoded and the driver writes the same
    masks as with --host_resize (used to raise AttributeError on the NumPy batch)."""
    from PIL import Image
    sizes = [(96, 192), (80, 100), (96, 192), (120, 90)]
    img_fns, lab_fns = [], []
    for i, (H, W) in enumerate(sizes):
        img = synth.synth_image(90 + i, H, W, integer_valued=True).astype(np.uint8).transpose(1, 2, 0)
        if i == 1:
            img = np.concatenate([img, np.full((H, W, 1), 255, np.uint8)], axis=2)      # RGBA: alpha dropped
        fn = str(tmp_path / ('mix_%06d_000019_leftImg8bit.png' % i))
        Image.fromarray(img).save(fn)
        lf = str(tmp_path / ('mix_%06d_000019_gtFine_labelIds.png' % i))
        Image.fromarray(synth.synth_gt_labels(90 + i, 64, 80)).save(lf)
        img_fns.append(fn); lab_fns.append(lf)
    (tmp_path / 'imgs.txt').write_text('\n'.join(img_fns) + '\n')
    (tmp_path / 'labs.txt').write_text('\n'.join(lab_fns) + '\n')
    outs = []
    for extra in ([], ['--host_resize']):
        out = tmp_path / ('out' + str(len(outs)))
        argv = ['--superpixel_method', 'slic', '--n_slic_segments', '20', '--n_clusters', '2',
                '--resize_shape', '64', '80', '--batchsize', '2', '--out_dir', str(out),
                '--img_file_list', str(tmp_path / 'imgs.txt'), '--label_file_list', str(tmp_path / 'labs.txt'),
                '--arch', 'drn_d_22', '--pool_mode', 'mean', '--no_figure'] + extra
        assert mods.cli.main_labelled(argv) == 0
        outs.append(out)
    for fn in img_fns:
        base = os.path.splitext(os.path.basename(fn))[0]
        assert np.array_equal(np.load(outs[0] / (base + '.npy')), np.load(outs[1] / (base + '.npy'))), base


def test_bench_two_ranks_on_one_gpu(tmp_path):
    """bench.py's N > 1 path end to end (sharding, barrier, max-over-ranks timing, record
    all_gather) with two ranks sharing this box's single GPU over gloo."""
    import subprocess
    env = dict(os.environ, SPA_DIST_BACKEND='gloo', SPA_BENCH_SAME_DEVICE='1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', '29611', os.path.join(ROOT, 'bench.py'),
           '--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '2', '--height', '128', '--width', '256',
           '--n_slic_segments', '40', '--drn_sub_batch', '2', '--full', '--no_cpu_baseline']
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1                                   # rank 0 only
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['scaling'] == 'weak' and d['value'] > 0
    assert d['quality']['records_gathered'] == 4             # 2 ranks x 2 images
    assert d['roofline']['bound'] in ('hbm', 'mfma', 'latency') and 'cpu_baseline' not in d
    assert d['roofline']['ms_per_step'] == max(k['ms_per_step'] for k in d['kernels'].values())
    h = d['host_to_host']                                    # SURVEY 8d's region, second timed loop
    assert h['value'] > 0 and h['images_downloaded'] == 2 * 2 * 2
    # round 5: multi-GPU bookkeeping of the line (per-rank rates, the gather's time on each rank, where the ranks sit) and the
    # same region on float32 matrix instructions
    m = d['multi_gpu']
    assert m['ranks'] == 2 and m['backend'] == 'gloo' and m['records_gathered'] == m['records_expected'] == 4
    assert len(m['per_rank_images_per_sec']) == 2 and all(v > 0 for v in m['per_rank_images_per_sec'])
    assert len(m['gather_ms_per_rank']) == 2 and m['rank_devices'] == [0, 0]          # SPA_BENCH_SAME_DEVICE: both on cuda:0
    assert d['exact_fp32_value'] > 0 and d['dtype'].startswith('f32 as 2 x f16')
    assert d['full'] and d['device_resident_value'] > 0                # --full: the device-resident loop ran too


def test_bench_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with no launcher environment starts its two ranks itself (torchrun as a child of
    a process that never touched the GPU) and forwards rank 0's single line with n_gpus = 2."""
    import subprocess
    env = {k: v for k, v in os.environ.items()
           if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(SPA_DIST_BACKEND='gloo', SPA_BENCH_SAME_DEVICE='1')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1',
           '--batch', '2', '--height', '128', '--width', '256', '--n_slic_segments', '40', '--drn_sub_batch', '2',
           '--no_host_loop']
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['value'] > 0 and d['quality']['records_gathered'] == 4
    assert 'cpu_baseline' not in d                           # rank 0 at N = 1 only


def test_bench_dumps_the_same_outputs_run_after_run(tmp_path):
    """`bench.py --dump-outputs DIR` writes what the headline loop returned for its last batch; two runs with the same
    arguments write the same arrays, and --steps is the number of timed steps.  A plain run (no --full) measures the
    headline loop alone."""
    import subprocess
    B, H, W, steps = 2, 128, 256, 3
    dumps = []
    for run in range(2):
        d = tmp_path / ('run%d' % run)
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1',
               '--batch', str(B), '--height', str(H), '--width', str(W), '--n_slic_segments', '40',
               '--dump-outputs', str(d)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert line['steps'] == steps and line['ms_per_step'] > 0
        assert line['host_to_host']['images_downloaded'] == B * steps
        assert line['dumped_outputs']['dir'] == str(d)
        assert not line['full'] and 'cpu_baseline' not in line
        assert line['exact_fp32_value'] is None and line['device_resident_value'] is None
        dumps.append({p[:-4]: np.load(str(d / p)) for p in sorted(os.listdir(str(d)))})
    a, b = dumps
    assert sorted(a) == ['assignment', 'cluster', 'descriptors', 'features', 'n_superpixels', 'prior', 'road', 'superpixels']
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a['cluster'].shape == a['road'].shape == a['superpixels'].shape == (B, H, W)
    n = int(a['n_superpixels'].sum())
    assert a['descriptors'].shape[0] == a['prior'].shape[0] == a['assignment'].shape[0] == n > 0
    assert set(np.unique(a['assignment'])) <= {0.0, 1.0} and set(np.unique(a['road'])) <= {0.0, 1.0}
    for name in a:
        assert np.array_equal(a[name], b[name]), name


def test_host_stream_matches_device_resident_path(mods, synth):
    """pipeline.HostStream (pinned host batches -> masks in pinned host memory, uploads and downloads
    double buffered on copy streams) returns exactly what the device-resident path returns, batch
    after batch, for pinned and for pageable inputs and a short last batch."""
    args = _args(pool_mode='mean', n_slic_segments=40)
    H, W, B = 96, 160, 3
    model = mods.drn.create_drn('drn_d_22', device='cuda')
    pipe = mods.pipeline.LabelPipeline(args, model, mods.ops.engine())
    batches = [synth.synth_batch([70 + 3 * s + i for i in range(B)], H, W) for s in range(5)]
    batches[4] = batches[4][:2]                              # the driver's last batch may be short
    expect = []
    for b in batches:
        r = pipe.run(b)
        expect.append((r.cluster.cpu().numpy(), r.road.cpu().numpy()))
    hs = mods.pipeline.HostStream(pipe, B, H, W)
    seen = []
    feed = [torch.from_numpy(b).pin_memory() if i % 2 == 0 else b for i, b in enumerate(batches)]
    for cl, road, res in hs.process(iter(feed)):
        seen.append((cl.copy(), road.copy()))
    assert len(seen) == len(expect)
    for (c0, r0), (c1, r1) in zip(expect, seen):
        assert np.array_equal(c0, c1) and np.array_equal(r0, r1)
    pipe.eng.raise_on_status()


def test_stream_layouts_return_the_same_bits(mods, synth, monkeypatch):
    """The pipeline on one stream, on two (superpixel branch beside the DRN forward: the default) and with the batch's tail on
    the second stream as well (SPA_PIPE_TAIL_AUX=1, run(join=False)) returns the same labels, descriptors, clusters and
    masks, bit for bit, batch after batch and run after run — at the size where kernels of the two streams really share
    compute units (12 x 1024 x 2048, batches enqueued back to back without a host synchronisation).  Round 4 found a variant
    of k_slic_assign that was bit exact alone and changed ~100 labels per batch beside the stem kernel: this is the test
    that sees such a thing (tools/determinism_check.py is the same loop at 30 images)."""
    import hashlib
    args = _args(pool_mode='mean', n_slic_segments=200)
    B, H, W = 12, 1024, 2048
    model = mods.drn.create_drn('drn_d_22', device='cuda')
    batches = [torch.from_numpy(synth.synth_batch([500 + 40 * k + i for i in range(B)], H, W)).cuda() for k in range(2)]

    def digest(t):
        return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    seen = {}
    for name, overlap, tail in (('one stream', False, '0'), ('two streams', True, '0'), ('two streams, tail on the second', True, '1')):
        monkeypatch.setenv('SPA_PIPE_TAIL_AUX', tail)
        pipe = mods.pipeline.LabelPipeline(args, model, mods.ops.engine(), overlap=overlap)
        assert pipe.tail_on_aux == (tail == '1')
        for rep in range(3):
            rs = [pipe.run(batches[k % 2], check_status=False, join=False) for k in range(4)]
            torch.cuda.synchronize()
            for k, r in enumerate(rs):
                n = int(r.offsets[-1])
                d = (digest(r.labels), digest(r.X[:n]), digest(r.assign[:n]), digest(r.cluster), digest(r.road))
                seen.setdefault(k % 2, set()).add(d)
        pipe.eng.raise_on_status()
    assert all(len(v) == 1 for v in seen.values()), {k: len(v) for k, v in seen.items()}


@pytest.mark.parametrize('mode,B', [('mean_k2', 30), ('anchor_k2', 12), ('mean_k4', 12)])
def test_fifty_batches_per_stream_layout_same_bits(mods, synth, monkeypatch, mode, B):
    """The statistical form of the guard above: the co-residency miscompare of round 4 showed up in 50-160
    labels of SOME batches, so every stream layout runs 50 back-to-back full-size batches (two distinct batches alternating,
    no host synchronisation between them where the mode allows it) and every result must equal, bit for bit on the device, the
    first result of the first layout — the default bench batch (30 images, mean pooling, k = 2), anchor mode, and k = 4 (both
    generators re-seeded before every run, so that runs are comparable: `LabelPipeline.reseed`)."""
    H, W = 1024, 2048
    args = _args(pool_mode='anchor' if mode == 'anchor_k2' else 'mean', n_slic_segments=200, n_clusters=4 if mode == 'mean_k4' else 2)
    model = mods.drn.create_drn('drn_d_22', device='cuda')
    batches = [torch.from_numpy(synth.synth_batch([900 + 40 * k + i for i in range(B)], H, W)).cuda() for k in range(2)]
    layouts = [('one stream', False, '0'), ('two streams', True, '0')]
    if mode != 'anchor_k2':
        layouts.append(('two streams, tail on the second', True, '1'))
    want = {}
    runs = bad = 0
    for name, overlap, tail in layouts:
        monkeypatch.setenv('SPA_PIPE_TAIL_AUX', tail)
        pipe = mods.pipeline.LabelPipeline(args, model, mods.ops.engine(), overlap=overlap)
        for rep in range(0, 50, 5):
            rs = []
            for k in range(rep, rep + 5):
                pipe.reseed()
                rs.append(pipe.run(batches[k % 2], check_status=False, join=False))
            torch.cuda.synchronize()
            for k, r in zip(range(rep, rep + 5), rs):
                n = int(r.offsets[-1])
                got = (r.labels, r.X[:n], r.assign[:n], r.cluster, r.road)
                if k % 2 not in want:
                    want[k % 2] = tuple(t.clone() for t in got)
                    continue
                runs += 1
                if not all(torch.equal(a, b) for a, b in zip(got, want[k % 2])):
                    bad += 1
                    print('%s, run %d: differs from the first result (labels %d, cluster pixels %d)'
                          % (name, k, int((got[0] != want[k % 2][0]).sum()), int((got[3] != want[k % 2][3]).sum())))
            del rs
        pipe.eng.raise_on_status()
    print('%s: %d runs compared over %d layouts, %d differ' % (mode, runs, len(layouts), bad))
    assert bad == 0


@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('shape', [(2, 64, 96), (1, 100, 75), (3, 33, 130)])
def test_fused_drn_d_stem_matches_convolution_path(mods, shape, split):
    """libspalign's float32-MFMA stem kernel (normalise + layer0 + layer1 of DRN-D) against the
    MIOpen convolutions + separate epilogues it replaces: float32 rounding-level agreement on
    layer1's output and on the final map, including image sizes that are not tile multiples."""
    B, H, W = shape
    model = mods.drn.create_drn('drn_d_22', None, device='cuda', dtype=torch.float32, seed=3)
    assert model._stem is not None
    x = torch.rand(B, 3, H, W, device='cuda') * 255
    model.use_fused_stem = False
    _, ref = model.batch_predict(x)
    ref = [m.clone() for m in ref]
    model.use_fused_stem = True
    saved = mods.drn._EPILOGUE['split_gemm']
    mods.drn._EPILOGUE['split_gemm'] = split        # the stem on the 16-bit matrix cores (two half-precision planes) or float32 MFMA
    try:
        _, got = model.batch_predict(x)
        for i in (0, 1, 7):
            scale = float(ref[i].abs().max())
            assert float((got[i] - ref[i]).abs().max()) <= 2e-5 * scale
        # layer1's output against float64 convolutions of the same normalised image: float32 rounding level either way
        eng = mods.drn._EPILOGUE['engine']
        l1 = eng.drn_stem_d(x.float().contiguous(), *model._stem, dtype=torch.float32, split=split)
        xn = ((x.double() / 255.0) - torch.tensor([0.485, 0.456, 0.406], device='cuda', dtype=torch.float64).view(1, 3, 1, 1)) \
            / torch.tensor([0.229, 0.224, 0.225], device='cuda', dtype=torch.float64).view(1, 3, 1, 1)
        c0, c1 = model.layer0[0], model.layer1[0]
        r = torch.relu(torch.nn.functional.conv2d(xn, c0.weight.double(), c0.bias.double(), 1, 3))
        r = torch.relu(torch.nn.functional.conv2d(r, c1.weight.double(), c1.bias.double(), 1, 1))
        assert float((l1.double() - r).abs().max()) <= 3e-6 * float(r.abs().max())
    finally:
        mods.drn._EPILOGUE['split_gemm'] = saved


def test_fused_stem_in_bf16_mode(mods):
    """bf16 network: the stem kernel computes in float32 and stores bf16; compared with the bf16
    MIOpen path it replaces, against the float32 network as the common reference."""
    B, H, W = 2, 64, 96
    ref_model = mods.drn.create_drn('drn_d_22', None, device='cuda', dtype=torch.float32, seed=5)
    model = mods.drn.create_drn('drn_d_22', None, device='cuda', dtype=torch.bfloat16, seed=5)
    x = torch.rand(B, 3, H, W, device='cuda') * 255
    _, ref = ref_model.batch_predict(x)
    model.use_fused_stem = False
    _, plain = model.batch_predict(x)
    plain = [m.float() for m in plain]
    model.use_fused_stem = True
    _, fused = model.batch_predict(x)
    assert fused[0].dtype == torch.bfloat16
    for i in (0, 7):
        scale = float(ref[i].abs().max())
        e_plain = float((plain[i] - ref[i]).abs().max()) / scale
        e_fused = float((fused[i].float() - ref[i]).abs().max()) / scale
        assert e_fused <= max(1.25 * e_plain, 2e-2), (i, e_fused, e_plain)


@pytest.mark.parametrize('case', [
    # B, Cin, Cout, H, W, dilation, residual, relu       (channel tiles of 256 / 128 / 64; ragged pixel tiles;
    (2, 64, 256, 9, 300, 1, False, True),              #  dilations 1 / 2 / 4 at the image borders)
    (1, 128, 512, 20, 256, 4, True, True),
    (2, 256, 256, 7, 70, 2, True, False),
    (1, 64, 128, 11, 513, 1, True, True),
    (2, 128, 128, 6, 40, 2, False, True),
    (1, 64, 64, 13, 260, 1, True, True),
    (1, 192, 64, 5, 33, 4, False, False),
])
def test_conv3x3_bf16_against_float32_convolution(mods, case):
    """spa_conv3x3_bf16 (bf16 MFMA implicit GEMM, float32 accumulation, bias / residual / ReLU fused) against
    torch's float32 convolution of the SAME bf16 operands: the only difference allowed is the float32
    accumulation order and the final rounding to bf16 (tolerance: one bf16 ulp of the largest output, 2^-8)."""
    B, Cin, Cout, H, W, dil, res, relu = case
    eng = mods.engine.default_engine()
    g = torch.Generator(device='cuda').manual_seed(Cin * 7 + Cout + H)
    x = torch.randn((B, Cin, H, W), device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn((Cout, Cin, 3, 3), device='cuda', generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(torch.bfloat16)
    bias = torch.randn((Cout,), device='cuda', generator=g)
    r = None
    if res:
        r = torch.randn((B, Cout, H, W), device='cuda', generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wt = w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin).contiguous()
    y = eng.conv3x3_bf16(x, wt, bias, r, relu, dil)
    assert y.dtype == torch.bfloat16 and y.shape == (B, Cout, H, W)
    ref = torch.nn.functional.conv2d(x.float(), w.float(), bias, 1, dil, dil)
    if res:
        ref = ref + r.float()
    if relu:
        ref = torch.relu(ref)
    scale = float(ref.abs().max())
    assert float((y.float() - ref).abs().max()) <= scale * 2.0 ** -8
    eng.raise_on_status()
