#!/usr/bin/env python
"""The demo-video stage (utils/create_demovideo.py, superpixel-align_amd/demovideo.py) on the MI355X and its host: what
a frame costs on the device, in the fused mask-and-blend launch, in the decode workers and in the encoders, and what
label_frames makes of them end to end.  One process, one session, a warm-up before every timed window:

  (a) chain       the device chain alone on a resident batch (segnet_train_input, the network with logits=True,
                  segnet_overlay), in device events, for float32, split planes and bf16
  (b) overlay     Engine.segnet_overlay alone in device events, with the bytes it moves (3 read + 3 written + 1 mask
                  byte per pixel, and the scores) and the resulting rate
  (c) fused       segnet_overlay and one download of the mask and the blended frames into pinned memory, against the
                  composition of existing pieces it replaces (segnet_score, the mask's download, demovideo.blend_host
                  per frame), wall time per batch, the two alternating over --rounds rounds, with the spread
  (d) decode      one worker's time per frame (decode_worker.png_into, into a slab), run in this process
  (e) encode      one thread's time per frame for the JPEG (demovideo.encode_jpeg) and for the label PNG
  (f) end to end  label_frames per frame at loader_procs 0 and N, with and without a video, per dtype, beside
                  bound_ms = max((a) / B, (d) / N, (e) / encode_threads)

on B frames of 1024 x 2048 run at 512 x 1024 and labelled at 1024 x 2048, from synthetic PNGs
(tests/segnet_train_synth.image).  Synthetic frames carry noise and compress less than photographs; (d), (e) and (f)
share that.  The loops' times include the fill of the pipeline.

  python tools/demovideo_bench.py [--procs 0 4 8] [--n_frames 24] [--out profiles/demovideo_b4.json]
"""
import argparse
import importlib
import json
import os
import shutil
import sys
import tempfile
import time
from multiprocessing import shared_memory

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
torch = segnet = dv = dw = engine = None


def _imports():
    """in main() only: the spawned workers import this file as their main module and must stay light"""
    global torch, segnet, dv, dw, engine
    import torch
    segnet = importlib.import_module('superpixel-align_amd.segnet')
    dv = importlib.import_module('superpixel-align_amd.demovideo')
    dw = importlib.import_module('superpixel-align_amd.decode_worker')
    engine = importlib.import_module('superpixel-align_amd.engine')


def event_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def wall_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def decode_seconds(fns, shape, n):
    """(d): one worker's work for one frame, into a slab as the workers do it"""
    ishape = tuple(shape) + (3,)
    shm = shared_memory.SharedMemory(create=True, size=int(np.prod(ishape)) + 64)
    try:
        s = 0.0
        for i in range(n + 1):
            t0 = time.perf_counter()
            got = dw.png_into((shm.name, 0, ishape, 'RGB', fns[i % len(fns)]))
            t1 = time.perf_counter()
            assert got == (ishape, 'RGB')
            if i:                                            # the first call imports the plugin
                s += t1 - t0
    finally:
        dw._SHM.pop(shm.name).close()
        shm.close()
        shm.unlink()
    return s / n


def encode_seconds(frames, masks, out_root, n):
    """(e): one thread's JPEG encode of a blended frame and PNG write of its label"""
    j = p = 0.0
    for i in range(n + 1):
        frame = dv.blend_host(frames[i % len(frames)], masks[i % len(masks)])
        t0 = time.perf_counter()
        data = dv.encode_jpeg(frame)
        t1 = time.perf_counter()
        dv.write_label_png(os.path.join(out_root, 'enc%d.png' % i), masks[i % len(masks)])
        t2 = time.perf_counter()
        if i:
            j += t1 - t0
            p += t2 - t1
    return j / n, p / n, len(data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--procs', type=int, nargs='+', default=[0, 4, 8])
    ap.add_argument('--n_frames', type=int, default=24)
    ap.add_argument('--frame', type=int, nargs=2, default=[1024, 2048])
    ap.add_argument('--input_shape', type=int, nargs=2, default=[512, 1024])
    ap.add_argument('--encode_threads', type=int, default=4)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    _imports()
    import segnet_train_synth as syn
    from segnet_bench import random_params
    torch.cuda.set_device(0)
    eng = engine.default_engine()
    B, n = a.batch, a.n_frames
    in_shape, shape = tuple(a.input_shape), tuple(a.frame)
    H, W = shape
    root = tempfile.mkdtemp(prefix='demovideo_bench_')
    try:
        t0 = time.perf_counter()
        rng = np.random.default_rng(0)
        os.makedirs(os.path.join(root, 'demoVideo', 'synth'))
        host_frames = []
        for i in range(n):
            img, _ = syn.image(H, W, rng)
            with open(os.path.join(root, 'demoVideo', 'synth', 'synth_000000_%06d_leftImg8bit.png' % i), 'wb') as f:
                f.write(syn.png(img))
            if i < B:
                host_frames.append(img)
        fns = dv.demo_frames(os.path.join(root, 'demoVideo'))
        print('wrote %d frames of %dx%d in %.1f s' % (n, H, W, time.perf_counter() - t0), flush=True)
        params = random_params(0)
        out = {'what': 'utils/create_demovideo.py: the device chain, the fused mask-and-blend launch, decode, encode, '
                       'label_frames end to end',
               'batch': B, 'frame': list(shape), 'input': list(in_shape), 'frames': n,
               'encode_threads': a.encode_threads, 'cpus_visible': len(os.sched_getaffinity(0)),
               'device': torch.cuda.get_device_name(0)}

        frames_h = np.stack(host_frames)
        frames_d = torch.from_numpy(frames_h).cuda()
        modes = {'fp32': {}, 'split_planes': {'split_planes': True}, 'bf16': {'dtype': 'bf16'}}
        models = {m: segnet.SegNetBasic(params, shape, engine=eng, **kw) for m, kw in modes.items()}
        z = models['fp32'].forward(eng.segnet_train_input(frames_d, in_shape), logits=True)

        # (b) the launch alone
        ov_ms = [event_ms(lambda: eng.segnet_overlay(z, frames_d), a.iters) for _ in range(a.rounds)]
        nbytes = B * (7 * H * W + 2 * 4 * in_shape[0] * in_shape[1])
        med = float(np.median(ov_ms))
        out['overlay'] = {'ms_rounds': ov_ms, 'ms': med, 'spread_ms': max(ov_ms) - min(ov_ms), 'bytes': nbytes,
                          'tb_per_s': nbytes / (med * 1e-3) / 1e12}
        print('overlay %.3f ms per batch, %.2f TB/s' % (med, out['overlay']['tb_per_s']), flush=True)

        # (c) fused against the pieces it replaces, alternating
        pin_m = torch.empty((B, H, W), dtype=torch.uint8).pin_memory()
        pin_b = torch.empty((B, H, W, 3), dtype=torch.uint8).pin_memory()

        def fused():
            mask, blended = eng.segnet_overlay(z, frames_d)
            pin_m.copy_(mask, non_blocking=True)
            pin_b.copy_(blended, non_blocking=True)
            torch.cuda.synchronize()

        def unfused():
            mask, _ = eng.segnet_score(z, shape)
            pin_m.copy_(mask, non_blocking=True)
            torch.cuda.synchronize()
            mh = pin_m.numpy()
            return [dv.blend_host(frames_h[j], mh[j]) for j in range(B)]

        f_ms, u_ms = [], []
        for _ in range(a.rounds):
            f_ms.append(wall_ms(fused, 3))
            u_ms.append(wall_ms(unfused, 3))
        spread = max(max(f_ms) - min(f_ms), max(u_ms) - min(u_ms))
        fm, um = float(np.median(f_ms)), float(np.median(u_ms))
        out['fused_vs_unfused'] = {'fused_ms_rounds': f_ms, 'unfused_ms_rounds': u_ms, 'fused_ms': fm, 'unfused_ms': um,
                                   'spread_ms': spread, 'fused_faster_beyond_spread': bool(fm + spread < um)}
        print('fused %.2f ms, unfused %.2f ms per batch (spread %.2f)' % (fm, um, spread), flush=True)
        masks_h = [m.copy() for m in pin_m.numpy()]

        # (a) the chain per dtype
        out['chain_ms_per_batch'] = {}
        for m, model in models.items():
            def chain():
                eng.segnet_overlay(model.forward(eng.segnet_train_input(frames_d, in_shape), logits=True), frames_d)
            out['chain_ms_per_batch'][m] = event_ms(chain, 5)
        print('chain', out['chain_ms_per_batch'], flush=True)

        # (d), (e)
        dec_s = decode_seconds(fns, shape, 6)
        jpg_s, png_s, jpg_bytes = encode_seconds(host_frames, masks_h, root, 6)
        out['decode'] = {'frame_s': dec_s}
        out['encode'] = {'jpeg_s': jpg_s, 'label_png_s': png_s, 'jpeg_bytes': jpg_bytes}
        print('decode %.1f ms, jpeg %.1f ms, label png %.1f ms per frame' % (dec_s * 1e3, jpg_s * 1e3, png_s * 1e3),
              flush=True)

        # (f) end to end
        out['label_frames'] = {}
        for m, model in models.items():
            rows = {}
            for p in a.procs:
                for with_video in (False, True):
                    def run(frames, tag):
                        d = os.path.join(root, 'out_' + tag)
                        stats = {}
                        video = dv.MjpegAviWriter(os.path.join(root, tag + '.avi'), (W, H),
                                                  encode_threads=a.encode_threads) if with_video else None
                        try:
                            dv.label_frames(model, frames, d, in_shape, shape, B, p, video, a.encode_threads, stats=stats)
                        finally:
                            if video is not None:
                                video.close()
                        shutil.rmtree(d, ignore_errors=True)
                        return stats
                    run(fns[:B], 'warm')
                    s = run(fns, 'timed')
                    enc_s = png_s + (jpg_s if with_video else 0.0)
                    terms = {'chain': out['chain_ms_per_batch'][m] / B, 'decode': dec_s * 1e3 / max(p, 1),
                             'encode': enc_s * 1e3 / a.encode_threads}
                    r = {'ms_per_frame': s['loop_s'] * 1e3 / n, 'loader_wait_ms': s['loader_wait_s'] * 1e3 / n,
                         'device_wait_ms': s['device_wait_s'] * 1e3 / n, 'output_ms': s['output_s'] * 1e3 / n,
                         'host_batches': s['n_host_batches'], 'bound_ms': max(terms.values()),
                         'bound_is': max(terms, key=terms.get)}
                    r['ms_over_bound'] = r['ms_per_frame'] / r['bound_ms']
                    rows['procs%d_%s' % (p, 'video' if with_video else 'labels')] = r
                    print('%s loader_procs %d %s: %.1f ms per frame (loader %.1f, device %.1f, output %.1f), bound %.1f '
                          'ms (%s)' % (m, p, 'video' if with_video else 'labels', r['ms_per_frame'], r['loader_wait_ms'],
                                       r['device_wait_ms'], r['output_ms'], r['bound_ms'], r['bound_is']), flush=True)
            out['label_frames'][m] = rows
    finally:
        shutil.rmtree(root, ignore_errors=True)
    s = json.dumps(out, indent=2)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fp:
            fp.write(s + '\n')


if __name__ == '__main__':
    main()
