#!/usr/bin/env python
"""The input stage of SegNet-Basic training on the MI355X and its host: what train_segnet.py's loop costs per step with
and without --loader_procs, against the step alone and the decode rate of the workers.  One process, one session:

  (a) plain_ms     wall time per iteration of today's loop: get_example for every image of the batch on the main
                   thread (decode, Pillow resize, label, augmentation), upload, step
  (b) loader[N]    wall time per iteration with segnet_loader.TrainLoader on N workers and the device stage, split
                   into the time the loop waits in loader.next() and the step
  (c) step_ms      the step alone on a resident batch
  (d) decode       one worker's time per example (decode_worker.decode_into + label_into, into a slab), run in this
                   process, and the ceiling N / that of N workers
  (e) kernels      device-event times of Engine.segnet_train_input and segnet_train_label on one batch with the bytes
                   they move (input: the frames read, the horizontal pass written and read, the images written;
                   label: masks read, int32 written), and the upload of a registered shared-memory slab of one
                   batch.  The times are per call of a loop of calls: a kernel shorter than the host's time to issue a
                   call is marked launch_bound and gets no rate

for float32 and bf16 at B images of 512 x 1024 from full-size (1024 x 2048) synthetic zips
(tests/segnet_train_synth.write; --random, MomentumSGD).  For every N the result gives bound_ms = max(step_ms,
B / (N / decode_s)) and loader_ms / bound_ms.  Synthetic frames carry noise and compress less than photographs, so
their PNGs decode slower than Cityscapes frames do; (a), (b) and (d) share that.

  python tools/segnet_train_loader_bench.py [--procs 4 8 16] [--steps 12] [--n_images 24] [--out FILE.json]

With --device_cache_gb G the tool measures train_segnet.py --device_cache_gb instead (cache_main), in one session, per
dtype with --fused_bn: row (c); per N of --cache_procs the uncached row (b) and the cached loader's step time and
next() wait in epoch 1 and in epochs 2-3 (an epoch is n_images / batch iterations), with the bytes cached; the uncached
row (b) at N = 16; one train_segnet.evaluate pass over --n_val frames with the uncached label loader, then the first and
the second pass of the cached one; and the _ptrs input kernels against the contiguous ones on one batch, alternating
over 5 rounds (median and spread of the per-call device time).

  python tools/segnet_train_loader_bench.py --device_cache_gb 2 --out profiles/segnet_train_cache_b4.json
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
torch = st = sl = dw = engine = None


def _imports():
    """in main() only: the spawned workers import this file as their main module and must stay light"""
    global torch, st, sl, dw, engine
    import torch
    st = importlib.import_module('superpixel-align_amd.segnet_train')
    sl = importlib.import_module('superpixel-align_amd.segnet_loader')
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


def plain_loop(ds, it, trainer, dev, warmup, steps):
    """train_segnet.py's default loop body"""
    times = {'prepare': 0.0, 'step': 0.0}
    for k in range(warmup + steps):
        if k == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        ta = time.perf_counter()
        batch = [ds.get_example(i) for i in it.next_indices()]
        img = torch.from_numpy(np.stack([b[0] for b in batch])).to(dev)
        lab = torch.from_numpy(np.stack([b[1] for b in batch])).to(dev)
        tb = time.perf_counter()
        trainer.step(img, lab)
        if k >= warmup:
            times['prepare'] += tb - ta
            times['step'] += time.perf_counter() - tb
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    return {'ms': total * 1e3 / steps, 'prepare_ms': times['prepare'] * 1e3 / steps,
            'step_ms': times['step'] * 1e3 / steps}


def loader_loop(ds, it, trainer, n_procs, warmup, steps, cache=None):
    t_start = time.perf_counter()
    loader = sl.TrainLoader(ds, np.arange(len(ds)), it, n_procs, sl.DeviceStage(ds, trainer.eng), cache=cache)
    started = time.perf_counter() - t_start
    try:
        waits = steps_t = 0.0
        for k in range(warmup + steps):
            if k == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            ta = time.perf_counter()
            img, lab, _ = loader.next()
            tb = time.perf_counter()
            trainer.step(img, lab)
            if k >= warmup:
                waits += tb - ta
                steps_t += time.perf_counter() - tb
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        loader.close()
    return {'ms': total * 1e3 / steps, 'next_ms': waits * 1e3 / steps, 'step_ms': steps_t * 1e3 / steps,
            'batches_in_flight': loader.depth, 'slabs_pinned': loader.pinned, 'start_s': started,
            'host_batches': loader.n_host_batches}


def decode_seconds(ds, n):
    """one worker's work for one example, into a slab as the workers do it"""
    ishape, lshape = sl._first_shapes(ds)
    ibytes = int(np.prod(ishape))
    shm = shared_memory.SharedMemory(create=True, size=ibytes + int(np.prod(lshape)) * 4 + 64)
    try:
        img_s = lab_s = 0.0
        for i in range(n + 1):
            t0 = time.perf_counter()
            dw.decode_into((shm.name, 0, ishape, (ds.img_zip_fn, ds.img_fns[i % len(ds)])))
            t1 = time.perf_counter()
            dw.label_into((shm.name, ibytes, lshape, (ds.label_zip_fn, ds.label_fns[i % len(ds)])))
            t2 = time.perf_counter()
            if i:                                            # the first call opens the archives and imports the plugin
                img_s += t1 - t0
                lab_s += t2 - t1
    finally:
        dw._SHM.pop(shm.name).close()
        shm.close()
        shm.unlink()
    return img_s / n, lab_s / n


def kernel_rows(eng, B, src, dst, iters):
    """(e): device-event time per call over a loop of calls, so a row cannot go below the time the host needs to issue
    one call.  null_call_ms is that floor (the same entry point on 16 x 16 frames); a row within twice the floor is
    marked launch_bound and gets no rate, because its time says nothing about the bytes."""
    H, W = src
    h, w = dst
    g = torch.Generator(device='cuda').manual_seed(0)
    u8 = torch.randint(0, 256, (B, H, W, 3), generator=g, device='cuda', dtype=torch.uint8)
    masks = torch.randint(0, 2, (B, H, W), generator=g, device='cuda', dtype=torch.uint8)
    scores = torch.rand((B, 2, H, W), generator=g, device='cuda')
    shift = torch.randn((B, 3), generator=g, device='cuda', dtype=torch.float64)
    flip = torch.tensor([1, 0] * B, device='cuda', dtype=torch.uint8)[:B].contiguous()
    tiny_u8, tiny_m = u8[:, :16, :16].contiguous(), masks[:, :16, :16].contiguous()

    def row(fn, null_fn, nbytes):
        ms, null = event_ms(fn, iters), event_ms(null_fn, iters)
        bound = ms < 2 * null
        return {'ms': ms, 'null_call_ms': null, 'bytes': nbytes, 'launch_bound': bound,
                'gb_per_s': None if bound else nbytes / (ms * 1e-3) / 1e9}

    rows = {}
    rows['train_input'] = row(lambda: eng.segnet_train_input(u8, dst, shift, flip, 'pil'),
                              lambda: eng.segnet_train_input(tiny_u8, (8, 8), shift, flip, 'pil'),
                              B * (H * W * 3 + 2 * 3 * H * w * 4 + 3 * h * w * 4))
    null_label = lambda: eng.segnet_train_label(tiny_m, (8, 8), flip, 'pil')
    rows['train_label_masks'] = row(lambda: eng.segnet_train_label(masks, dst, flip, 'pil'), null_label,
                                    B * (h * w + h * w * 4))
    rows['train_label_scores'] = row(lambda: eng.segnet_train_label(scores, dst, flip, 'pil'), null_label,
                                     B * 2 * (h * w * 4 + h * w * 4))
    return rows


def slab_upload_row(eng, nbytes, iters):
    """the loader's own upload: a shared-memory slab registered as the device stage registers it, copied on a stream"""
    stage = sl.DeviceStage(None, eng)
    shm = shared_memory.SharedMemory(create=True, size=nbytes)
    handle = stage.register(shm)
    try:
        ms = event_ms(lambda: handle['t'].to(eng.device, non_blocking=True), iters)
        return {'ms': ms, 'bytes': nbytes, 'gb_per_s': nbytes / (ms * 1e-3) / 1e9, 'pinned': handle['pinned']}
    finally:
        torch.cuda.synchronize()
        stage.unregister(handle)
        shm.close()
        shm.unlink()


def cached_epochs(ds, trainer, n_procs, cache, B, epochs=3):
    """the cached loader from its first batch on: per epoch the wall time per iteration, the next() wait and the step"""
    per = len(ds) // B
    loader = sl.TrainLoader(ds, np.arange(len(ds)), st.ShuffledIterator(len(ds), B), n_procs,
                            sl.DeviceStage(ds, trainer.eng), cache=cache)
    rows = []
    try:
        for _ in range(epochs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            waits = 0.0
            for _ in range(per):
                ta = time.perf_counter()
                img, lab, _ = loader.next()
                waits += time.perf_counter() - ta
                trainer.step(img, lab)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            rows.append({'ms': total * 1e3 / per, 'next_ms': waits * 1e3 / per})
    finally:
        loader.close()
    later = rows[1:]
    return {'epoch1': rows[0], 'epochs2_3': {'ms': float(np.mean([r['ms'] for r in later])),
                                             'next_ms': float(np.mean([r['next_ms'] for r in later]))},
            'per_epoch': rows, 'iterations_per_epoch': per, 'hits': loader.cache_hits, 'misses': loader.cache_misses}


def ptrs_rows(eng, B, src, dst, iters, rounds=5):
    """the _ptrs input kernels against the contiguous ones on the same batch, alternating; per-call device ms"""
    H, W = src
    g = torch.Generator(device='cuda').manual_seed(0)
    u8 = torch.randint(0, 256, (B, H, W, 3), generator=g, device='cuda', dtype=torch.uint8)
    masks = torch.randint(0, 2, (B, H, W), generator=g, device='cuda', dtype=torch.uint8)
    shift = torch.randn((B, 3), generator=g, device='cuda', dtype=torch.float64)
    flip = torch.tensor([1, 0] * B, device='cuda', dtype=torch.uint8)[:B].contiguous()
    tu = torch.tensor([u8[j].data_ptr() for j in range(B)], dtype=torch.int64, device='cuda')
    tm = torch.tensor([masks[j].data_ptr() for j in range(B)], dtype=torch.int64, device='cuda')
    fns = {'train_input': lambda: eng.segnet_train_input(u8, dst, shift, flip, 'pil'),
           'train_input_ptrs': lambda: eng.segnet_train_input_ptrs(tu, B, src, dst, shift, flip, 'pil'),
           'train_label_masks': lambda: eng.segnet_train_label(masks, dst, flip, 'pil'),
           'train_label_masks_ptrs': lambda: eng.segnet_train_label_ptrs(tm, B, src, np.uint8, dst, flip, 'pil')}
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(event_ms(fn, iters))
    return {k: {'median_ms': float(np.median(v)), 'min_ms': min(v), 'max_ms': max(v)} for k, v in ms.items()}


def evaluate_rows(trainer, valid, eval_shape, B, n_procs, budget):
    """one validation pass with the uncached label loader, then the first and the second pass of the cached one"""
    fc = importlib.import_module('superpixel-align_amd.frame_cache')
    train_segnet = importlib.import_module('train_segnet')
    ids = list(range(len(valid)))

    def timed(loader):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = train_segnet.evaluate(trainer, valid, eval_shape, B, ids, loader=loader)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, rep
    out = {}
    loader = sl.LabelLoader(valid, ids, B, n_procs, sl.DeviceLabelStage(trainer.eng))
    try:
        timed(loader)                                          # the predictor is built and the workers are warm
        out['uncached_ms'], want = timed(loader)
    finally:
        loader.close()
    cache = fc.DeviceFrameCache(budget, trainer.eng.device)
    loader = sl.LabelLoader(valid, ids, B, n_procs, sl.DeviceLabelStage(trainer.eng), cache=cache)
    try:
        out['cached_first_ms'], r1 = timed(loader)
        out['cached_second_ms'], r2 = timed(loader)
    finally:
        loader.close()
        cache.close()
    out.update(n_images=len(ids), procs=n_procs, bytes_cached=cache.counters()['bytes'],
               same_report=bool(json.dumps(want, sort_keys=True) == json.dumps(r1, sort_keys=True) ==
                                json.dumps(r2, sort_keys=True)))
    return out


def cache_main(a):
    _imports()
    import segnet_train_synth as syn
    fc = importlib.import_module('superpixel-align_amd.frame_cache')
    segnet = importlib.import_module('superpixel-align_amd.segnet')
    torch.cuda.set_device(0)
    eng = engine.Engine(0)
    dev = eng.device
    B, shape = a.batch, tuple(a.input_shape)
    budget = int(a.device_cache_gb * (1 << 30))
    root = tempfile.mkdtemp(prefix='segnet_cache_bench_')
    try:
        z = syn.write(root, a.n_images, a.n_val, a.frame[0], a.frame[1])
        ds = st.ZippedEstimatedCityscapesDataset(z[0], z[1], shape, True, False)
        valid = segnet.ZippedCityscapesRoadDataset(z[2], z[3], shape)
        img_s, lab_s = decode_seconds(ds, 6)
        out = {'what': 'train_segnet.py --device_cache_gb: the cached loader against --loader_procs N and the step alone',
               'batch': B, 'frame': list(a.frame), 'input': list(shape), 'random': True, 'optimizer': 'MomentumSGD',
               'fused_bn': True, 'n_images': a.n_images, 'budget_bytes': budget,
               'cpus_visible': len(os.sched_getaffinity(0)), 'device': torch.cuda.get_device_name(0),
               'decode': {'image_s': img_s, 'label_s': lab_s},
               'kernels': ptrs_rows(eng, B, tuple(a.frame), shape, 100), 'dtypes': {}}
        for dtype in a.dtypes:
            np.random.seed(0)
            trainer = st.SegNetTrainer(st.init_params(0), st.MomentumSGD(0.01, weight_decay=0.0005),
                                       st.softmax_cross_entropy, engine=eng, dtype=dtype, fused_bn=True)
            batch = [ds.get_example(i) for i in range(B)]
            img = torch.from_numpy(np.stack([b[0] for b in batch])).to(dev)
            lab = torch.from_numpy(np.stack([b[1] for b in batch])).to(dev)
            for _ in range(2):
                trainer.step(img, lab)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                trainer.step(img, lab)
            torch.cuda.synchronize()
            row = {'step_ms': (time.perf_counter() - t0) * 1e3 / a.steps, 'uncached': {}, 'cached': {}}
            for n in sorted(set(a.cache_procs + [16])):
                row['uncached'][str(n)] = loader_loop(ds, st.ShuffledIterator(len(ds), B), trainer, n, a.warmup,
                                                      a.steps)
            for n in a.cache_procs:
                cache = fc.DeviceFrameCache(budget, dev)
                try:
                    r = cached_epochs(ds, trainer, n, cache, B)
                finally:
                    cache.close()
                r.update(cache.counters())
                r['cached_over_step'] = r['epochs2_3']['ms'] / row['step_ms']
                row['cached'][str(n)] = r
                print(dtype, 'N %d: step %.1f ms, uncached %.1f ms, cached epoch 1 %.1f ms, epochs 2-3 %.1f ms '
                      '(next %.2f ms), %d bytes' % (n, row['step_ms'], row['uncached'][str(n)]['ms'], r['epoch1']['ms'],
                                                    r['epochs2_3']['ms'], r['epochs2_3']['next_ms'], r['bytes']),
                      flush=True)
            row['uncached16_over_step'] = row['uncached']['16']['ms'] / row['step_ms']
            row['evaluate'] = evaluate_rows(trainer, valid, tuple(a.frame), B, 4, budget)
            out['dtypes'][dtype] = row
            del trainer
    finally:
        shutil.rmtree(root, ignore_errors=True)
    s = json.dumps(out, indent=2)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fp:
            fp.write(s + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--procs', type=int, nargs='+', default=[4, 8, 16])
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--plain_steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--n_images', type=int, default=24)
    ap.add_argument('--frame', type=int, nargs=2, default=[1024, 2048])
    ap.add_argument('--input_shape', type=int, nargs=2, default=[512, 1024])
    ap.add_argument('--dtypes', nargs='+', default=['fp32', 'bf16'], choices=['fp32', 'bf16'])
    ap.add_argument('--out', default=None)
    ap.add_argument('--device_cache_gb', type=float, default=0.0,
                    help='measure train_segnet.py --device_cache_gb with this budget instead (see above)')
    ap.add_argument('--cache_procs', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--n_val', type=int, default=8)
    a = ap.parse_args()
    if a.device_cache_gb > 0:
        return cache_main(a)
    _imports()
    import segnet_train_synth as syn
    torch.cuda.set_device(0)
    eng = engine.Engine(0)
    dev = eng.device
    B, shape = a.batch, tuple(a.input_shape)
    root = tempfile.mkdtemp(prefix='segnet_loader_bench_')
    try:
        t0 = time.perf_counter()
        z = syn.write(root, a.n_images, 1, a.frame[0], a.frame[1])
        print('wrote %d frames of %dx%d in %.1f s' % (a.n_images, a.frame[0], a.frame[1], time.perf_counter() - t0),
              flush=True)
        ds = st.ZippedEstimatedCityscapesDataset(z[0], z[1], shape, True, False)
        img_s, lab_s = decode_seconds(ds, 6)
        out = {'what': 'train_segnet.py input stage: plain loop, --loader_procs N, the step alone, decode, kernels',
               'batch': B, 'frame': list(a.frame), 'input': list(shape), 'random': True, 'optimizer': 'MomentumSGD',
               'cpus_visible': len(os.sched_getaffinity(0)), 'device': torch.cuda.get_device_name(0),
               'decode': {'image_s': img_s, 'label_s': lab_s, 'examples_per_s_per_worker': 1.0 / (img_s + lab_s)},
               'kernels': kernel_rows(eng, B, tuple(a.frame), shape, 200), 'dtypes': {}}
        out['kernels']['slab_upload'] = slab_upload_row(eng, B * a.frame[0] * a.frame[1] * 4, 50)   # frames + masks
        per_example = img_s + lab_s
        for dtype in a.dtypes:
            np.random.seed(0)
            trainer = st.SegNetTrainer(st.init_params(0), st.MomentumSGD(0.01, weight_decay=0.0005),
                                       st.softmax_cross_entropy, engine=eng, dtype=dtype)
            batch = [ds.get_example(i) for i in range(B)]
            img = torch.from_numpy(np.stack([b[0] for b in batch])).to(dev)
            lab = torch.from_numpy(np.stack([b[1] for b in batch])).to(dev)
            for _ in range(2):
                trainer.step(img, lab)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                trainer.step(img, lab)
            torch.cuda.synchronize()
            step_ms = (time.perf_counter() - t0) * 1e3 / a.steps
            row = {'step_ms': step_ms,
                   'plain': plain_loop(ds, st.ShuffledIterator(len(ds), B), trainer, dev, 1, a.plain_steps),
                   'loader': {}}
            print(dtype, 'step %.1f ms, plain loop %.1f ms' % (step_ms, row['plain']['ms']), flush=True)
            for n in a.procs:
                r = loader_loop(ds, st.ShuffledIterator(len(ds), B), trainer, n, a.warmup, a.steps)
                r['decode_ceiling_ms'] = B * per_example * 1e3 / n
                r['bound_ms'] = max(step_ms, r['decode_ceiling_ms'])
                r['bound_is'] = 'step' if step_ms >= r['decode_ceiling_ms'] else 'decode'
                r['ms_over_bound'] = r['ms'] / r['bound_ms']
                r['speedup_over_plain'] = row['plain']['ms'] / r['ms']
                row['loader'][str(n)] = r
                print(dtype, 'loader_procs %d: %.1f ms (next %.1f + step %.1f), bound %.1f ms (%s), x%.2f of it'
                      % (n, r['ms'], r['next_ms'], r['step_ms'], r['bound_ms'], r['bound_is'], r['ms_over_bound']),
                      flush=True)
            out['dtypes'][dtype] = row
            del trainer
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
