#!/usr/bin/env python
"""The input and output stages of SegNet-Basic labelling and validation on the MI355X and its host: what
labels_from_segnet.save_labels and train_segnet.evaluate cost per image with and without --loader_procs, against the
device chain alone, the decode rate of the workers and the host's output work.  One process, one session, a warm-up
before every timed window:

  (a) plain        wall time per image of save_labels' batch loop today (save_each=True, no figure)
  (b) loader[N]    the same with --loader_procs N, with the time the loop waits for the loader, waits for the device
                   and spends writing the outputs (the rest is issuing the launches)
  (c) chain        the device chain alone on a resident batch (resize, network, segnet_label_eval), for float32, split
                   planes and bf16
  (d) decode       one worker's time per frame and per labelIds image (decode_worker.png_into, into a slab), run in
                   this process, and the ceiling N / that of N workers
  (e) kernels      Engine.segnet_label_eval against the two launches it replaces (segnet_score, then confusion on an
                   int32 label): device events around loops of calls, the two forms alternating over --rounds rounds
                   in this process, with and without scores, each with the bytes it moves computed from the shapes;
                   a call shorter than twice the host's time to issue it is marked launch_bound and gets no rate
  (f) output       the host's output work per image: save_each=True, the two np.save calls of the mask and the JSON
                   line; save_each=False, the mask and the 16 MB float32 scores as run_train_rounds.label_worker
                   spools them
  (g) validation   one train_segnet.evaluate over the validation frames with and without a LabelLoader, against the
                   time of 50 training steps on a resident batch

at B images of 512 x 1024 evaluated at 1024 x 2048, from full-size synthetic zips (tests/segnet_train_synth.write).
For every N: bound_ms = max((c) / B, 1 / (N x the decode rate), (f)) per image, and (b) / bound_ms.  The loops' times
include the fill of the pipeline: the first batch's decode is never hidden.  Synthetic frames carry noise and compress
less than photographs; (a), (b), (d) and (g) share that.

  python tools/segnet_label_bench.py [--procs 4 8 16] [--n_images 24] [--out FILE.json]
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
torch = segnet = st = sl = dw = engine = lfs = train_segnet = None


def _imports():
    """in main() only: the spawned workers import this file as their main module and must stay light"""
    global torch, segnet, st, sl, dw, engine, lfs, train_segnet
    import torch
    segnet = importlib.import_module('superpixel-align_amd.segnet')
    st = importlib.import_module('superpixel-align_amd.segnet_train')
    sl = importlib.import_module('superpixel-align_amd.segnet_loader')
    dw = importlib.import_module('superpixel-align_amd.decode_worker')
    engine = importlib.import_module('superpixel-align_amd.engine')
    lfs = importlib.import_module('labels_from_segnet')
    train_segnet = importlib.import_module('train_segnet')


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


def decode_seconds(ds, n):
    """(d): one worker's work for one frame and one labelIds image, into a slab as the workers do it"""
    ishape, lshape = sl._first_png_shapes(ds)
    ibytes = int(np.prod(ishape))
    shm = shared_memory.SharedMemory(create=True, size=ibytes + int(np.prod(lshape)) + 64)
    try:
        img_s = lab_s = 0.0
        for i in range(n + 1):
            t0 = time.perf_counter()
            got = dw.png_into((shm.name, 0, ishape, 'RGB', (ds.img_zip_fn, ds.img_fns[i % len(ds)])))
            t1 = time.perf_counter()
            dw.png_into((shm.name, ibytes, lshape, 'L', (ds.label_zip_fn, ds.label_fns[i % len(ds)])))
            t2 = time.perf_counter()
            assert got == (ishape, 'RGB')
            if i:                                            # the first call opens the archives and imports the plugin
                img_s += t1 - t0
                lab_s += t2 - t1
    finally:
        dw._SHM.pop(shm.name).close()
        shm.close()
        shm.unlink()
    return img_s / n, lab_s / n


def save_labels_row(param_dir, z, out_root, name, n, B, shape, procs, **kw):
    """(a) / (b): a warm-up call over one batch, then the timed call over n images; per image, from the batch loop's
    own clock (no model load, no worker start)"""
    out = os.path.join(out_root, name)
    lfs.save_labels(param_dir, 1, 0, z[2], z[3], out + '_warm', 0, B, False, list(shape), save_each=True, figure=False,
                    batchsize=B, loader_procs=procs, **kw)
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lfs.save_labels(param_dir, 1, 0, z[2], z[3], out, 0, n, False, list(shape), save_each=True, figure=False,
                    batchsize=B, loader_procs=procs, loader_stats=stats, **kw)
    call_s = time.perf_counter() - t0
    row = {'ms_per_image': stats['loop_s'] * 1e3 / n, 'call_s': call_s}
    if procs:
        row.update({'loader_wait_ms': stats['loader_wait_s'] * 1e3 / n, 'device_wait_ms': stats['device_wait_s'] * 1e3 / n,
                    'output_ms': stats['output_s'] * 1e3 / n, 'host_batches': stats['n_host_batches'],
                    'slabs_pinned': stats['pinned']})
    shutil.rmtree(out, ignore_errors=True)
    shutil.rmtree(out + '_warm', ignore_errors=True)
    return row


def chain_ms(eng, params, B, frame, in_shape, shape, iters, **kw):
    """(c): resize -> network -> segnet_label_eval on a resident batch, ms per batch"""
    g = torch.Generator(device='cuda').manual_seed(0)
    u8 = torch.randint(0, 256, (B,) + tuple(frame) + (3,), generator=g, device='cuda', dtype=torch.uint8)
    ids = torch.randint(0, 34, (B,) + tuple(shape), generator=g, device='cuda', dtype=torch.uint8)
    model = segnet.SegNetBasic(params, shape, engine=eng, **kw)

    def run():
        eng.segnet_label_eval(model.forward(eng.resize_cvcubic_u8(u8, in_shape)), shape, ids)
    run()
    return event_ms(run, iters)


def kernel_rows(eng, B, in_shape, shape, iters, rounds):
    """(e): the fused launch against segnet_score + confusion, alternating round by round"""
    h, w = in_shape
    H, W = shape
    g = torch.Generator(device='cuda').manual_seed(1)
    prob = torch.softmax(torch.randn((B, 2, h, w), generator=g, device='cuda'), 1).contiguous()
    ids = torch.randint(0, 34, (B, H, W), generator=g, device='cuda', dtype=torch.uint8)
    gt = torch.from_numpy(segnet.label_mask(ids.cpu().numpy())).cuda()
    tiny_p, tiny_i = prob[:, :, :8, :8].contiguous(), ids[:, :8, :8].contiguous()
    tiny_g = gt[:, :8, :8].contiguous()
    rows = {}
    for want in (False, True):
        def fused():
            eng.segnet_label_eval(prob, shape, ids, want_scores=want)

        def pair():
            mask, _ = eng.segnet_score(prob, shape, want_scores=want)
            eng.confusion(mask, gt)

        def null_fused():
            eng.segnet_label_eval(tiny_p, (8, 8), tiny_i, want_scores=want)

        def null_pair():
            mask, _ = eng.segnet_score(tiny_p, (8, 8), want_scores=want)
            eng.confusion(mask, tiny_g)
        f_ms, p_ms = [], []
        for _ in range(rounds):
            f_ms.append(event_ms(fused, iters))
            p_ms.append(event_ms(pair, iters))
        nf, npair = event_ms(null_fused, iters), event_ms(null_pair, iters)
        common = B * (2 * h * w * 4 + H * W + (2 * H * W * 4 if want else 0))      # prob read, mask (and scores) written
        fb, pb = common + B * H * W, common + B * (H * W + H * W * 4)              # + ids read | + mask and int32 read

        def row(ms, null, nbytes):
            med = float(np.median(ms))
            bound = med < 2 * null
            return {'ms_rounds': ms, 'ms': med, 'spread_ms': max(ms) - min(ms), 'null_call_ms': null, 'bytes': nbytes,
                    'launch_bound': bound, 'gb_per_s': None if bound else nbytes / (med * 1e-3) / 1e9}
        r = {'label_eval': row(f_ms, nf, fb), 'score_plus_confusion': row(p_ms, npair, pb)}
        r['fused_over_pair'] = r['label_eval']['ms'] / r['score_plus_confusion']['ms']
        spread = max(r['label_eval']['spread_ms'], r['score_plus_confusion']['spread_ms'])
        r['fused_not_slower_within_spread'] = bool(r['label_eval']['ms'] <= r['score_plus_confusion']['ms'] + spread)
        rows['with_scores' if want else 'mask_only'] = r
    return rows


def output_rows(out_root, shape, n):
    """(f): the host's output work per image, on this file system"""
    rng = np.random.default_rng(0)
    mask = rng.random(tuple(shape)) > 0.5
    scores = rng.random((2,) + tuple(shape)).astype(np.float32)
    d = os.path.join(out_root, 'output')
    os.makedirs(d, exist_ok=True)
    line = {'img_fn': 'leftImg8bit/val/synth/x_leftImg8bit.png', 'road_iou': 0.5, 'train_args': {'model': 'basic'}}
    t = {'save_each': 0.0, 'spool': 0.0}
    for k in range(n + 1):
        t0 = time.perf_counter()
        np.save(os.path.join(d, 'm%d' % k), mask)
        np.save(os.path.join(d, 'm%d_scores' % k), mask)
        with open(os.path.join(d, 'result.json'), 'a') as fp:
            print(json.dumps(line), file=fp)
        t1 = time.perf_counter()
        np.save(os.path.join(d, 's%d.npy' % (2 * k)), mask)
        np.save(os.path.join(d, 's%d.npy' % (2 * k + 1)), scores)
        t2 = time.perf_counter()
        if k:
            t['save_each'] += t1 - t0
            t['spool'] += t2 - t1
    shutil.rmtree(d, ignore_errors=True)
    return {'save_each_ms': t['save_each'] * 1e3 / n, 'spool_scores_ms': t['spool'] * 1e3 / n}


def validation_row(eng, valid, shape, B, n, procs, steps):
    """(g): evaluate with and without the loader, and `steps` training steps on a resident batch"""
    trainer = st.SegNetTrainer(st.init_params(0), st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy,
                               engine=eng)
    g = torch.Generator().manual_seed(0)
    img = (torch.rand((B, 3) + tuple(valid.resize_shape), generator=g) * 255).cuda()
    lab = torch.randint(-1, 2, (B,) + tuple(valid.resize_shape), generator=g).cuda()
    for _ in range(2):
        trainer.step(img, lab)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        trainer.step(img, lab)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / 5
    ids = list(range(n))
    train_segnet.evaluate(trainer, valid, list(shape), B, ids[:B])            # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = train_segnet.evaluate(trainer, valid, list(shape), B, ids)
    plain_s = time.perf_counter() - t0
    row = {'images': n, 'plain_s': plain_s, 'step_ms': step_ms, 'steps': steps, 'steps_s': step_ms * steps * 1e-3,
           'loader': {}}
    for p in procs:
        loader = sl.LabelLoader(valid, ids, B, p, sl.DeviceLabelStage(eng))
        try:
            train_segnet.evaluate(trainer, valid, list(shape), B, ids, loader=loader)       # warm-up pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = train_segnet.evaluate(trainer, valid, list(shape), B, ids, loader=loader)
            s = time.perf_counter() - t0
        finally:
            loader.close()
        same = all(want[k] == got[k] or (want[k] != want[k] and got[k] != got[k]) for k in want)
        row['loader'][str(p)] = {'s': s, 'speedup': plain_s / s, 'same_report': bool(same)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--procs', type=int, nargs='+', default=[4, 8, 16])
    ap.add_argument('--n_images', type=int, default=24)
    ap.add_argument('--frame', type=int, nargs=2, default=[1024, 2048])
    ap.add_argument('--input_shape', type=int, nargs=2, default=[512, 1024])
    ap.add_argument('--eval_shape', type=int, nargs=2, default=[1024, 2048])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    _imports()
    import segnet_train_synth as syn
    from segnet_bench import random_params
    torch.cuda.set_device(0)
    eng = engine.default_engine()
    B, n = a.batch, a.n_images
    in_shape, shape = tuple(a.input_shape), tuple(a.eval_shape)
    root = tempfile.mkdtemp(prefix='segnet_label_bench_')
    try:
        t0 = time.perf_counter()
        z = syn.write(root, 0, n, a.frame[0], a.frame[1])
        print('wrote %d frames of %dx%d in %.1f s' % (n, a.frame[0], a.frame[1], time.perf_counter() - t0), flush=True)
        params = random_params(0)
        param_dir = os.path.join(root, 'run')
        os.makedirs(param_dir)
        with open(os.path.join(param_dir, 'args.txt'), 'w') as f:
            json.dump({'model': 'basic', 'input_shape': list(in_shape), 'batchsize': B}, f)
        with open(os.path.join(param_dir, 'snapshot_iter_1'), 'wb') as f:
            np.savez(f, **{segnet.PREFIX + k: v for k, v in params.items()})
        valid = segnet.ZippedCityscapesRoadDataset(z[2], z[3], in_shape)
        img_s, lab_s = decode_seconds(valid, 6)
        rate = 1.0 / (img_s + lab_s)
        out = {'what': 'labels_from_segnet.py / train_segnet.evaluate: plain loop, --loader_procs N, the device chain, '
                       'decode, the fused kernel, host output, validation',
               'batch': B, 'frame': list(a.frame), 'input': list(in_shape), 'eval_shape': list(shape), 'images': n,
               'cpus_visible': len(os.sched_getaffinity(0)), 'device': torch.cuda.get_device_name(0),
               'decode': {'frame_s': img_s, 'label_ids_s': lab_s, 'images_per_s_per_worker': rate}}
        print('decode: frame %.1f ms, labelIds %.1f ms' % (img_s * 1e3, lab_s * 1e3), flush=True)
        out['output'] = output_rows(root, shape, 6)
        out['kernels'] = kernel_rows(eng, B, in_shape, shape, a.iters, a.rounds)
        for k, r in out['kernels'].items():
            print('kernels %s: fused %.3f ms, pair %.3f ms' % (k, r['label_eval']['ms'], r['score_plus_confusion']['ms']),
                  flush=True)
        modes = {'fp32': {}, 'split_planes': {'split_planes': True}, 'bf16': {'dtype': 'bf16'}}
        out['chain_ms_per_batch'] = {m: chain_ms(eng, params, B, a.frame, in_shape, shape, 5, **kw)
                                     for m, kw in modes.items()}
        print('chain', out['chain_ms_per_batch'], flush=True)
        out['save_labels'] = {}
        for m, kw in modes.items():
            procs = a.procs if m == 'fp32' else a.procs[:1]
            row = {'plain': save_labels_row(param_dir, z, root, 'plain', n, B, shape, 0, **kw), 'loader': {}}
            print(m, 'plain %.1f ms per image' % row['plain']['ms_per_image'], flush=True)
            chain = out['chain_ms_per_batch'][m] / B
            for p in procs:
                r = save_labels_row(param_dir, z, root, 'loader%d' % p, n, B, shape, p, **kw)
                terms = {'chain': chain, 'decode': 1e3 / (p * rate), 'output': out['output']['save_each_ms']}
                r['bound_ms'] = max(terms.values())
                r['bound_is'] = max(terms, key=terms.get)
                r['decode_ceiling_ms'] = terms['decode']
                r['ms_over_bound'] = r['ms_per_image'] / r['bound_ms']
                r['speedup_over_plain'] = row['plain']['ms_per_image'] / r['ms_per_image']
                row['loader'][str(p)] = r
                print(m, 'loader_procs %d: %.1f ms per image (loader %.1f, device %.1f, output %.1f), bound %.1f ms (%s)'
                      % (p, r['ms_per_image'], r['loader_wait_ms'], r['device_wait_ms'], r['output_ms'], r['bound_ms'],
                         r['bound_is']), flush=True)
            out['save_labels'][m] = row
        out['validation'] = validation_row(eng, valid, shape, B, n, a.procs, 50)
        print('validation', out['validation'], flush=True)
        sl_row = out['save_labels']
        out['holds'] = {
            'loader_below_plain_at_every_n': all(r['ms_per_image'] < row['plain']['ms_per_image']
                                                 for row in sl_row.values() for r in row['loader'].values()),
            'validation_with_loader_below_without': all(r['s'] < out['validation']['plain_s']
                                                        for r in out['validation']['loader'].values()),
            'fused_not_slower_than_pair_within_spread': all(r['fused_not_slower_within_spread']
                                                            for r in out['kernels'].values())}
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
