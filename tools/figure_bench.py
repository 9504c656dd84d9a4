#!/usr/bin/env python
"""The drivers' overview figures, drawn by matplotlib on the host and composed on the device (--figure_renderer device,
csrc/spa_figure.hip + csrc/spa_jpeg.hip), in one process and one session, the variants alternating over --rounds
rounds, every figure with its spread (max - min over the rounds).  Sources of 1024 x 2048: synthetic road scenes, their
road masks as the estimate, labelIds images with road = 7, and a four-level cluster image.

  (a) matplotlib  cli.save_figure per image on one thread and on 8 threads, labels_from_segnet._save_figure per image
                  on one thread (it draws through pyplot's global state, so it has no threaded form): the path every
                  driver takes by default, unchanged, and the baseline
  (b) device      Engine.figure_compose + Engine.jpeg_encode per batch of 4 and of 30 in device events (2x2 and 1x3),
                  the source bytes read, the canvas bytes written and the scan bytes that come down; and the host's
                  jpeg.assemble + write per figure
  (c) labelled    batch_spalign_kmeans.py end to end on --n_images synthetic frames with the launchers' flags
                  (felzenszwalb, 224 x 224) in batches of --batchsize: --figure_renderer matplotlib, device, and
                  --no_figure, in images per second of the whole call (model, first batch and all); every timed run
                  follows an untimed run of one batch of its own kind

`device_faster_beyond_spread` is true only where the device figure plus the larger spread is still below the baseline.

  python tools/figure_bench.py [--rounds 5] [--n_images 24] [--batchsize 8] [--out profiles/figure_device.json]
"""
import argparse
import contextlib
import importlib
import io
import json
import os
import shutil
import sys
import tempfile
import time
import types
import zipfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
H, W = 1024, 2048


def summary(rounds):
    return {'rounds': [float(v) for v in rounds], 'median': float(np.median(rounds)),
            'spread': float(max(rounds) - min(rounds))}


def faster(dev, base):
    return bool(dev['median'] + max(dev['spread'], base['spread']) < base['median'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--n_images', type=int, default=24)
    ap.add_argument('--batchsize', type=int, default=8)
    ap.add_argument('--skip', nargs='*', default=[], choices=['matplotlib', 'kernels', 'labelled'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import segnet_train_synth as syn
    cli = importlib.import_module('superpixel-align_amd.cli')
    figure = importlib.import_module('superpixel-align_amd.figure')
    jpeg = importlib.import_module('superpixel-align_amd.jpeg')
    png = importlib.import_module('superpixel-align_amd.png')
    engine = importlib.import_module('superpixel-align_amd.engine')
    lfs = importlib.import_module('labels_from_segnet')
    torch.cuda.set_device(0)
    eng = engine.default_engine()
    R = max(a.rounds, 1)
    root = tempfile.mkdtemp(prefix='figure_bench_')
    out = {'what': 'overview figures: matplotlib on the host against --figure_renderer device', 'source': [H, W],
           'rounds': R, 'cpus_visible': len(os.sched_getaffinity(0)), 'device': torch.cuda.get_device_name(0)}
    try:
        # ---- four scenes: frame, estimate (the scene's road mask), labelIds, clusters
        rng = np.random.default_rng(0)
        frames, roads, ids, clusters = [], [], [], []
        for _ in range(4):
            img, m = syn.image(H, W, rng)
            frames.append(np.ascontiguousarray(img))
            roads.append(m.astype(np.uint8))
            ids.append(np.where(m, 7, 26).astype(np.uint8))
            clusters.append(((np.arange(H)[:, None] // 256 + np.arange(W)[None, :] // 512) % 4 * (1 - m)).astype(np.uint8))
        img_dir = os.path.join(root, 'imgs')
        os.makedirs(img_dir)
        img_fns, lab_fns = [], []
        img_png = [syn.png(f) for f in frames]
        lab_png = [syn.png(i) for i in ids]
        for i in range(a.n_images):
            img_fns.append(os.path.join(img_dir, 'synth_%06d_000019_leftImg8bit.png' % i))
            lab_fns.append(os.path.join(img_dir, 'synth_%06d_000019_gtFine_labelIds.png' % i))
            for fn, data in ((img_fns[-1], img_png[i % 4]), (lab_fns[-1], lab_png[i % 4])):
                with open(fn, 'wb') as f:
                    f.write(data)
        for name, fns in (('imgs.txt', img_fns), ('labs.txt', lab_fns)):
            with open(os.path.join(root, name), 'w') as f:
                f.write('\n'.join(fns) + '\n')

        # ---- (a) matplotlib
        if 'matplotlib' not in a.skip:
            fig_dir = os.path.join(root, 'mpl')
            os.makedirs(fig_dir)
            args = types.SimpleNamespace(out_dir=fig_dir)
            zfn = os.path.join(root, 'imgs.zip')
            with zipfile.ZipFile(zfn, 'w') as zf:
                for i in range(4):
                    zf.writestr('s/synth_%d.png' % i, img_png[i])
            ds = types.SimpleNamespace(img_zf=zipfile.ZipFile(zfn), img_fns=['s/synth_%d.png' % i for i in range(4)],
                                       _open=lambda: None)

            def labelled(j):
                k = j % 4
                cli.save_figure(args, frames[k], roads[k], cli.create_label_mask(ids[k]), clusters[k], 'f%d.png' % j)

            def segnet_fig(j):
                k = j % 4
                lfs._save_figure(ds, k, roads[k].astype(bool), cli.create_label_mask(ids[k]), fig_dir)

            def per_image_s(fn, n, threads):
                t0 = time.perf_counter()
                if threads == 1:
                    for j in range(n):
                        fn(j)
                else:
                    with ThreadPoolExecutor(threads) as pool:
                        list(pool.map(fn, range(n)))
                return (time.perf_counter() - t0) / n
            res = {'save_figure_1thread_s': [], 'save_figure_8threads_s': [], 'segnet_save_figure_1thread_s': []}
            labelled(0)
            segnet_fig(0)
            for _ in range(R):
                res['save_figure_1thread_s'].append(per_image_s(labelled, 2, 1))
                res['save_figure_8threads_s'].append(per_image_s(labelled, 8, 8))
                res['segnet_save_figure_1thread_s'].append(per_image_s(segnet_fig, 2, 1))
            out['matplotlib'] = {k: summary(v) for k, v in res.items()}
            out['matplotlib']['file_bytes'] = {'save_figure': os.path.getsize(os.path.join(fig_dir, 'f0.png')),
                                               'segnet_save_figure': os.path.getsize(os.path.join(fig_dir, 'synth_0.png'))}
            print('matplotlib', json.dumps({k: v.get('median', v) for k, v in out['matplotlib'].items()}), flush=True)

        # ---- (b) the kernels
        if 'kernels' not in a.skip:
            def event_ms(fn, iters=10):
                fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / iters
            dev = lambda arrs, B: torch.from_numpy(np.stack([arrs[j % 4] for j in range(B)])).cuda()
            luts = {k: torch.from_numpy(v).cuda() for k, v in
                    dict(overlay=figure.overlay(), on7=figure.two_colour([7]), on1=figure.two_colour([1]),
                         on0=figure.two_colour([0]), k4=figure.clusters(4)).items()}
            rows = {}
            for name, layout in (('2x2', (2, 2)), ('1x3', (1, 3))):
                for B in (4, 30):
                    f_d, r_d, i_d, c_d = dev(frames, B), dev(roads, B), dev(ids, B), dev(clusters, B)
                    if name == '2x2':
                        planes, tabs = [r_d, i_d, c_d, c_d], [luts['overlay'], luts['on7'], luts['k4'], luts['on0']]
                        distinct = 3
                    else:
                        planes, tabs = [r_d, i_d, r_d], [luts['overlay'], luts['on7'], luts['on1']]
                        distinct = 2
                    modes = [1] + [0] * (len(planes) - 1)
                    Hc, Wc = figure.canvas_shape(H, W, layout)
                    canvas = torch.empty((B, Hc, Wc, 3), dtype=torch.uint8, device='cuda')
                    compose = lambda: eng.figure_compose(f_d, planes, tabs, modes, layout, out=canvas)
                    res = {'compose_ms': [], 'jpeg_ms': []}
                    for _ in range(R):
                        res['compose_ms'].append(event_ms(compose))
                        res['jpeg_ms'].append(event_ms(lambda: eng.jpeg_encode(canvas)))
                    compose()
                    scans, nb = eng.jpeg_encode(canvas)
                    nb_h, scans_h = nb.cpu().numpy(), scans.cpu().numpy()
                    t0 = time.perf_counter()
                    for j in range(min(B, 4)):
                        png.write_file(os.path.join(root, 'dev_%s_%d.jpg' % (name, j)),
                                       jpeg.assemble(scans_h[j, :nb_h[j]].tobytes(), Hc, Wc, jpeg.DEFAULT_RI))
                    host_ms = (time.perf_counter() - t0) * 1e3 / min(B, 4)
                    want = figure.compose_host(frames[0][None], [p[:1].cpu().numpy() for p in planes],
                                               [t.cpu().numpy() for t in tabs], modes, layout)
                    assert np.array_equal(canvas[:1].cpu().numpy(), want)
                    row = {k: summary(v) for k, v in res.items()}
                    row.update(canvas=[Hc, Wc], source_bytes_read=B * H * W * (3 + len(planes)),
                               distinct_source_bytes=B * H * W * (3 + distinct), canvas_bytes_written=B * Hc * Wc * 3,
                               downloaded_bytes=int(nb_h.sum()), file_bytes_mean=float(nb_h.mean()) + len(jpeg.header(Hc, Wc, 4)) + 2,
                               host_assemble_write_ms_per_figure=host_ms)
                    row['device_ms_per_figure'] = summary([(c + j) / B for c, j in zip(res['compose_ms'], res['jpeg_ms'])])
                    rows['%s_B%d' % (name, B)] = row
                    print(name, B, json.dumps({k: (v['median'] if isinstance(v, dict) else v) for k, v in row.items()}),
                          flush=True)
            out['device_kernels'] = rows
            if 'matplotlib' in out:
                per_fig = lambda key: summary([v / 1e3 for v in rows[key]['device_ms_per_figure']['rounds']])
                out['device_faster_beyond_spread'] = {
                    'save_figure_1thread_s': faster(per_fig('2x2_B30'), out['matplotlib']['save_figure_1thread_s']),
                    'save_figure_8threads_s': faster(per_fig('2x2_B30'), out['matplotlib']['save_figure_8threads_s']),
                    'segnet_save_figure_1thread_s': faster(per_fig('1x3_B30'),
                                                           out['matplotlib']['segnet_save_figure_1thread_s'])}

        # ---- (c) the labelled driver
        if 'labelled' not in a.skip:
            variants = {'matplotlib': [], 'device': ['--figure_renderer', 'device'], 'no_figure': ['--no_figure']}

            def drive(name, n):
                argv = ['--superpixel_method', 'felzenszwalb', '--n_clusters', '4', '--n_anchors', '10', '--n_neighbors', '4',
                        '--batchsize', str(a.batchsize), '--use_feature_maps', '7', '--start_index', '0',
                        '--end_index', str(n), '--img_file_list', os.path.join(root, 'imgs.txt'),
                        '--label_file_list', os.path.join(root, 'labs.txt'), '--gpu', '0',
                        '--out_dir', os.path.join(root, 'out_' + name)] + variants[name]
                print('labelled %s, %d images ...' % (name, n), file=sys.stderr, flush=True)
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    cli.main_labelled(argv)
                return time.perf_counter() - t0
            for name in variants:
                drive(name, a.batchsize)                          # the model, the solvers, the buffers
            r = {name: [] for name in variants}
            for _ in range(R):
                for name in variants:
                    # matplotlib leaves the device idle for seconds: every timed run follows a short one of its own kind
                    drive(name, a.batchsize)
                    r[name].append(a.n_images / drive(name, a.n_images))
                print('labelled round', json.dumps({k: v[-1] for k, v in r.items()}), file=sys.stderr, flush=True)
            rows = {name: summary(v) for name, v in r.items()}
            d, m, nf = rows['device'], rows['matplotlib'], rows['no_figure']
            rows['device_faster_than_matplotlib_beyond_spread'] = bool(d['median'] - max(d['spread'], m['spread']) > m['median'])
            rows['device_over_no_figure'] = d['median'] / nf['median']
            rows['device_slower_than_no_figure_beyond_spread'] = bool(d['median'] + max(d['spread'], nf['spread']) < nf['median'])
            out['labelled_driver_images_per_s'] = dict(rows, n_images=a.n_images, batchsize=a.batchsize)
            print('labelled', json.dumps(rows), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    s = json.dumps(out, indent=2)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fp:
            fp.write(s + '\n')
    else:
        print(s)


if __name__ == '__main__':
    main()
