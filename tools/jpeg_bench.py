#!/usr/bin/env python
"""The demo movie's JPEG frames, on the host (Pillow, MjpegAviWriter.write) and on the device (--jpeg_encoder device,
csrc/spa_jpeg.hip), in one process and one session, the variants alternating over --rounds rounds, every figure with
its spread (max - min over the rounds).  Frames of 1024 x 2048: synthetic street frames with the road colour blended
in by Engine.segnet_overlay from a random-weight SegNet-Basic, batches of 4.

  (a) pillow      demovideo.encode_jpeg (quality 75) on 1, 4 and 8 threads: wall time per frame
  (b) device      Engine.jpeg_encode per batch of 4 in device events for every restart interval of --ri, the scan
                  bytes that come down against the frame's 6 MiB, the file size against Pillow's, and the host's
                  jpeg.assemble per frame
  (c) frames      demovideo.label_frames with the video, end to end per frame, at --loader_procs of --procs, per
                  encoder (the device one at the restart intervals of --frames_ri)

The baseline is (a) and the pillow rows of (c), never the new code; `device_faster_beyond_spread` is true only where
the device figure plus the larger spread is still below the baseline.

  python tools/jpeg_bench.py [--rounds 5] [--out profiles/jpeg_device.json]
"""
import argparse
import importlib
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
H, W = 1024, 2048


def summary(rounds):
    return {'rounds': [float(v) for v in rounds], 'median': float(np.median(rounds)),
            'spread': float(max(rounds) - min(rounds))}


def faster(dev, base):
    return bool(dev['median'] + max(dev['spread'], base['spread']) < base['median'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--n_frames', type=int, default=24)
    ap.add_argument('--ri', type=int, nargs='+', default=[1, 2, 4, 8, 32, 128])
    ap.add_argument('--frames_ri', type=int, nargs='+', default=None, help='default: jpeg.DEFAULT_RI')
    ap.add_argument('--procs', type=int, nargs='+', default=[4, 8])
    ap.add_argument('--skip', nargs='*', default=[], choices=['frames'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import segnet_train_synth as syn
    import jpeg_cases as jc
    from segnet_bench import random_params
    dv = importlib.import_module('superpixel-align_amd.demovideo')
    jpeg = importlib.import_module('superpixel-align_amd.jpeg')
    segnet = importlib.import_module('superpixel-align_amd.segnet')
    engine = importlib.import_module('superpixel-align_amd.engine')
    torch.cuda.set_device(0)
    eng = engine.default_engine()
    R = max(a.rounds, 5)
    frames_ri = a.frames_ri or [jpeg.DEFAULT_RI]
    root = tempfile.mkdtemp(prefix='jpeg_bench_')
    out = {'what': 'the demo movie\'s JPEG frames: Pillow on the host against --jpeg_encoder device', 'frame': [H, W],
           'rounds': R, 'batch': 4, 'default_ri': jpeg.DEFAULT_RI, 'cpus_visible': len(os.sched_getaffinity(0)),
           'device': torch.cuda.get_device_name(0)}
    try:
        # ---- the frames, blended as the stage blends them
        rng = np.random.default_rng(0)
        os.makedirs(os.path.join(root, 'demoVideo', 'synth'))
        distinct = []
        for i in range(4):
            img, _ = syn.image(H, W, rng)
            distinct.append(syn.png(img))
        for i in range(a.n_frames):
            with open(os.path.join(root, 'demoVideo', 'synth', 'synth_000000_%06d_leftImg8bit.png' % i), 'wb') as f:
                f.write(distinct[i % 4])
        fns = dv.demo_frames(os.path.join(root, 'demoVideo'))
        model = segnet.SegNetBasic(random_params(0), (H, W), engine=eng)
        frames_d = torch.from_numpy(np.stack([dv.read_frame(fn) for fn in fns[:4]])).cuda()
        z = model.forward(eng.segnet_train_input(frames_d, (512, 1024)), logits=True)
        blended = eng.segnet_overlay(z, frames_d)[1]
        host = blended.cpu().numpy()

        def pillow_ms(n, threads):
            t0 = time.perf_counter()
            if threads == 1:
                for j in range(n):
                    dv.encode_jpeg(host[j % 4])
            else:
                with ThreadPoolExecutor(threads) as pool:
                    list(pool.map(lambda j: dv.encode_jpeg(host[j % 4]), range(n)))
            return (time.perf_counter() - t0) * 1e3 / n

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

        # ---- (a) (b), alternating
        res = {'pillow_%dthread_ms_per_frame' % t: [] for t in (1, 4, 8)}
        res.update({'device_kernels_B4_ri%d_ms' % ri: [] for ri in a.ri})
        res.update({'device_assemble_ri%d_ms_per_frame' % ri: [] for ri in a.ri})
        sizes = {}
        for _ in range(R):
            for t in (1, 4, 8):
                res['pillow_%dthread_ms_per_frame' % t].append(pillow_ms(8 * t, t))
            for ri in a.ri:
                res['device_kernels_B4_ri%d_ms' % ri].append(event_ms(lambda: eng.jpeg_encode(blended, ri)))
                o, nb = eng.jpeg_encode(blended, ri)
                nb_h = nb.cpu().numpy()
                scans = [o[j, :int(nb_h[j])].cpu().numpy() for j in range(4)]
                t0 = time.perf_counter()
                files = [jpeg.assemble(s.tobytes(), H, W, ri) for s in scans]
                res['device_assemble_ri%d_ms_per_frame' % ri].append((time.perf_counter() - t0) * 1e3 / 4)
                sizes[ri] = files
        pillow_files = [dv.encode_jpeg(host[j]) for j in range(4)]
        pillow_psnr = [jc.psnr(host[j], jc.decode(pillow_files[j])) for j in range(4)]
        row = {k: summary(v) for k, v in res.items()}
        row['pillow_file_bytes'] = float(np.mean([len(f) for f in pillow_files]))
        row['pillow_psnr_db'] = float(np.mean(pillow_psnr))
        row['frame_bytes'] = H * W * 3
        for ri in a.ri:
            files = sizes[ri]
            psnr = [jc.psnr(host[j], jc.decode(files[j])) for j in range(4)]          # Pillow opens every file
            row['device_ri%d' % ri] = {
                'file_bytes': float(np.mean([len(f) for f in files])),
                'file_bytes_over_pillow': float(np.mean([len(f) for f in files]) / row['pillow_file_bytes']),
                'downloaded_bytes_per_frame': float(np.mean([len(f) for f in files])) - len(jpeg.header(H, W, ri)) - 2 + 4,
                'psnr_db': float(np.mean(psnr)),
                'intervals_per_frame': -(-(H // 16) * (W // 16) // ri),
                'kernels_ms_per_frame': row['device_kernels_B4_ri%d_ms' % ri]['median'] / 4,
                'faster_beyond_spread_than_pillow_8thread': faster(
                    summary([v / 4 + h for v, h in zip(res['device_kernels_B4_ri%d_ms' % ri],
                                                       res['device_assemble_ri%d_ms_per_frame' % ri])]),
                    row['pillow_8thread_ms_per_frame'])}
        out['encode'] = row
        print('encode', json.dumps({k: (v['median'] if isinstance(v, dict) and 'median' in v else v)
                                    for k, v in row.items()}), flush=True)

        # ---- (c) label_frames with the video
        if 'frames' not in a.skip:
            size = (W, H)
            variants = [('pillow', {})] + [('device_ri%d' % ri, dict(jpeg_encoder='device', jpeg_restart=ri))
                                          for ri in frames_ri]
            variants.append(('device_ri%d_png_device' % frames_ri[0],
                             dict(jpeg_encoder='device', jpeg_restart=frames_ri[0], png_encoder='device')))
            variants.append(('pillow_png_device', dict(png_encoder='device')))

            def run(p, kw, n, stats=None):
                t0 = time.perf_counter()
                with dv.MjpegAviWriter(os.path.join(root, 'v.avi'), size) as w:
                    dv.label_frames(model, fns[:n], os.path.join(root, 'lf'), (512, 1024), (H, W), 4, p, video=w,
                                    stats=stats, **kw)
                return (time.perf_counter() - t0) * 1e3 / n, os.path.getsize(os.path.join(root, 'v.avi'))
            rows = {}
            for p in a.procs:
                r = {name: {'loop': [], 'call': [], 'output': [], 'device_wait': []} for name, _ in variants}
                avi = {}
                for name, kw in variants:                        # warm-up: workers' imports, buffers
                    run(p, kw, 8)
                for _ in range(R):
                    for name, kw in variants:
                        stats = {}
                        call_ms, avi[name] = run(p, kw, a.n_frames, stats)
                        r[name]['loop'].append(stats['loop_s'] * 1e3 / a.n_frames)
                        r[name]['call'].append(call_ms)
                        r[name]['output'].append(stats['output_s'] * 1e3 / a.n_frames)
                        r[name]['device_wait'].append(stats['device_wait_s'] * 1e3 / a.n_frames)
                rows['procs%d' % p] = {name: {'loop_ms_per_frame': summary(r[name]['loop']),
                                              'call_ms_per_frame': summary(r[name]['call']),
                                              'output_ms_per_frame': summary(r[name]['output']),
                                              'device_wait_ms_per_frame': summary(r[name]['device_wait']),
                                              'avi_bytes': avi[name]} for name, _ in variants}
                for name, _ in variants[1:]:
                    base = 'pillow_png_device' if name.endswith('png_device') and name != 'pillow_png_device' else 'pillow'
                    rows['procs%d' % p][name]['baseline'] = base
                    rows['procs%d' % p][name]['faster_beyond_spread'] = faster(
                        rows['procs%d' % p][name]['loop_ms_per_frame'], rows['procs%d' % p][base]['loop_ms_per_frame'])
                print('label_frames procs %d' % p, json.dumps(
                    {name: [v['loop_ms_per_frame']['median'], v['loop_ms_per_frame']['spread'],
                            v['output_ms_per_frame']['median']] for name, v in rows['procs%d' % p].items()}), flush=True)
            out['label_frames_with_video'] = dict(rows, n_frames=a.n_frames, batchsize=4)
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
