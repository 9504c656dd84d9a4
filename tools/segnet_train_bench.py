#!/usr/bin/env python
"""SegNet-Basic training on the MI355X: the time of one training step (segnet_train.SegNetTrainer.step, MomentumSGD)
and its images/s at B images of 512 x 1024, and for every layer the device-event time of each kernel pass (forward,
dgrad, wgrad) with its TFLOP/s from the layer shape (segnet.layer_flops: forward and dgrad each cost the layer's
forward FLOPs, wgrad too) against the matrix peak of the dtype: 157.3 TF float32, 16 x that (2516.8 TF dense) bf16.
Random weights and inputs: the time does not depend on the values.

  python tools/segnet_train_bench.py [--dtype fp32|bf16] [--split_planes] [--batch 4] [--iters 10] [--out ...]
  python tools/segnet_train_bench.py --fused_bn [--rounds 5] [--iters 10] [--out ...]
  rocprofv3 --kernel-trace --stats -- python tools/segnet_train_bench.py --fused_bn --trace bf16 --iters 3

--split_planes: the float32 step with its passes on split f16 planes (SegNetTrainer(split_planes=True)).  TFLOP/s
count the float32 FLOPs; the share of peak is that of the 16-bit dense peak (2516.8 TF) at 3 f16 products per float32
product.

--fused_bn: instead of the above, compare SegNetTrainer(fused_bn=True) with the default trainer in one process: for
each convolution family (fp32, bf16, split planes) the two trainers take --iters steps each, alternating, for --rounds
rounds; the figures are each mode's per-round step times, their median and spread (max - min over the rounds), and
whether the fused median is below the unfused one by more than the larger spread.  Then every kernel of
csrc/spa_segnet_train_bn.hip at the four resolutions of the network, with the bytes it has to move (from the shapes:
each operand read once, each output written once; the encoder sums count the selected quarter of y) over its
device-event time.  Writes profiles/segnet_train_bench_b4_fused.json unless --out says otherwise.

--data_parallel: the step of a data-parallel rank (segnet_train.RankGroup: BN statistics and gradients exchanged).
Under SPA_DIST_FORCE=1 on one GPU that is one RCCL rank, which times the exchanges' own cost; under torchrun one rank
of many.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
segnet = importlib.import_module('superpixel-align_amd.segnet')
st = importlib.import_module('superpixel-align_amd.segnet_train')
engine = importlib.import_module('superpixel-align_amd.engine')
PEAK_TF = {'fp32': 157.3, 'bf16': 16 * 157.3}


def event_ms(fn, iters):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


FAMILIES = (('fp32', {}), ('bf16', dict(dtype='bf16')), ('f16x3', dict(split_planes=True)))


def fused_kernel_rows(eng, B, H, W, iters, g):
    """every fused kernel at the network's four resolutions -> {kernel: {resolution: {ms, bytes, gb_per_s}}}"""
    rows = {}
    for lv in range(4):
        h_, w_ = H >> lv, W >> lv
        M = B * h_ * w_ * 64 * 4                                    # bytes of one full-resolution map
        y = torch.randn((B, h_, w_, 64), generator=g, device='cuda') * 1.5 + 0.3
        gr = torch.randn((B, h_, w_, 64), generator=g, device='cuda')
        gp = torch.randn((B, h_ // 2, w_ // 2, 64), generator=g, device='cuda')
        mean = y.mean((0, 1, 2))
        rstd = 1.0 / torch.sqrt(y.var((0, 1, 2), unbiased=False) + segnet.BN_EPS)
        gamma = torch.rand(64, generator=g, device='cuda') + 0.5
        beta = torch.rand(64, generator=g, device='cuda') * 0.2 - 0.1
        p, idx = eng.segnet_train_bn_forward(y, mean, rstd, gamma, beta, pool=True)
        sums = eng.segnet_train_bn_backward_sums(gr, y, mean, rstd)
        m = float(B * h_ * w_)
        o = torch.empty_like(y)
        calls = {
            'bn_forward_decoder': (2 * M, lambda: eng.segnet_train_bn_forward(y, mean, rstd, gamma, beta, out=o)),
            'bn_forward_encoder': (M + M // 4 + M // 16,
                                   lambda: eng.segnet_train_bn_forward(y, mean, rstd, gamma, beta, pool=True, out=p,
                                                                       out_idx=idx)),
            'bn_backward_sums_decoder': (2 * M, lambda: eng.segnet_train_bn_backward_sums(gr, y, mean, rstd, out=sums)),
            'bn_backward_sums_encoder': (3 * (M // 4) + M // 16,
                                         lambda: eng.segnet_train_bn_backward_sums(gp, y, mean, rstd, idx, p, out=sums)),
            'bn_backward_dy_decoder': (3 * M, lambda: eng.segnet_train_bn_backward_dy(gr, y, mean, rstd, gamma, sums, m,
                                                                                    out=o)),
            'bn_backward_dy_encoder': (2 * M + 2 * (M // 4) + M // 16,
                                       lambda: eng.segnet_train_bn_backward_dy(gp, y, mean, rstd, gamma, sums, m, idx, p,
                                                                               out=o)),
        }
        if lv == 0:                                                 # the classifier runs at full resolution only
            wc = torch.randn((2, 64), generator=g, device='cuda') / 4
            bc = torch.zeros(2, device='cuda')
            ds = torch.randn((B, h_, w_, 2), generator=g, device='cuda')
            sc = torch.empty((B, h_, w_, 2), device='cuda')
            calls['classifier_forward'] = (M + M // 32, lambda: eng.segnet_train_classifier_forward(y, wc, bc, out=sc))
            calls['classifier_backward'] = (2 * M + M // 32,
                                            lambda: eng.segnet_train_classifier_backward(ds, y, wc, out=o))
        for name, (nbytes, fn) in calls.items():
            ms = event_ms(fn, iters)
            rows.setdefault(name, {})['%dx%d' % (h_, w_)] = {'ms': ms, 'bytes': nbytes,
                                                             'gb_per_s': nbytes / (ms * 1e-3) / 1e9}
        del y, gr, gp, p, idx, o
        torch.cuda.empty_cache()
    return rows


def fused_main(a):
    """the --fused_bn comparison (see the module docstring)"""
    B, H, W = a.batch, a.height, a.width
    torch.cuda.set_device(0)
    eng = engine.Engine(0)
    g = torch.Generator(device='cuda').manual_seed(0)
    img = torch.rand((B, 3, H, W), generator=g, device='cuda') * 255
    t = torch.randint(0, 2, (B, H, W), generator=g, device='cuda')
    if a.trace:                       # under rocprofv3 --kernel-trace --stats: one warm-up and --iters fused steps
        tr = st.SegNetTrainer(st.init_params(0), st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy,
                              engine=eng, fused_bn=True, **dict(FAMILIES)[a.trace])
        for _ in range(a.iters + 1):
            tr.step(img, t)
        torch.cuda.synchronize()
        return
    out = {'batch': B, 'input': [H, W], 'iters_per_round': a.iters, 'rounds': a.rounds, 'families': {}}

    def timed(tr):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            tr.step(img, t)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.iters

    for fam, kw in FAMILIES:
        trs = {mode: st.SegNetTrainer(st.init_params(0), st.MomentumSGD(0.01, weight_decay=0.0005),
                                      st.softmax_cross_entropy, engine=eng, fused_bn=mode == 'fused', **kw)
               for mode in ('unfused', 'fused')}
        first = {mode: tr.step(img, t) for mode, tr in trs.items()}       # warm-up, and the two modes' first losses
        for tr in trs.values():
            tr.step(img, t)
        ms = {'unfused': [], 'fused': []}
        for _ in range(a.rounds):
            for mode in ('unfused', 'fused'):
                ms[mode].append(timed(trs[mode]))
        row = {'first_loss': first}
        for mode, v in ms.items():
            row[mode] = {'round_ms': v, 'median_ms': float(np.median(v)), 'spread_ms': max(v) - min(v)}
        gain = row['unfused']['median_ms'] - row['fused']['median_ms']
        row['gain_ms'] = gain
        row['faster_by_more_than_spread'] = bool(gain > max(row['unfused']['spread_ms'], row['fused']['spread_ms']))
        out['families'][fam] = row
        del trs
        torch.cuda.empty_cache()
    out['kernels'] = fused_kernel_rows(eng, B, H, W, a.iters, g)
    out['device'] = torch.cuda.get_device_name(0)
    s = json.dumps(out, indent=2)
    print(s)
    path = a.out or os.path.join(ROOT, 'profiles', 'segnet_train_bench_b4_fused.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as fp:
        fp.write(s + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fused_bn', action='store_true')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--trace', default=None, choices=['fp32', 'bf16', 'f16x3'],
                    help='with --fused_bn: only --iters fused steps of this family after one warm-up (for a kernel trace)')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--split_planes', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--data_parallel', action='store_true')
    a = ap.parse_args()
    if a.fused_bn:
        return fused_main(a)
    B, H, W = a.batch, a.height, a.width
    if a.split_planes and a.dtype != 'fp32':
        ap.error('--split_planes does not combine with --dtype %s' % a.dtype)
    sfx = '_f16x3' if a.split_planes else ('_bf16' if a.dtype == 'bf16' else '')
    peak = PEAK_TF['bf16'] / 3 if a.split_planes else PEAK_TF[a.dtype]     # float32 FLOP/s at 3 f16 products each
    group = None
    if a.data_parallel:
        dist = importlib.import_module('superpixel-align_amd.dist')
        dist.init()
        if torch.distributed.is_initialized():
            group = st.RankGroup()
        eng = engine.default_engine()
    else:
        torch.cuda.set_device(0)
        eng = engine.Engine(0)
    fwd, dgrad, wgrad = (getattr(eng, 'segnet_train_' + k + sfx) for k in ('forward', 'dgrad', 'wgrad'))
    flops = segnet.layer_flops(H, W)
    g = torch.Generator(device='cuda').manual_seed(0)
    rows = {}
    for i, name in enumerate(segnet.LAYERS):
        if i < 4:
            h_, w_ = H >> i, W >> i
            x = (torch.rand((B, 3, H, W), generator=g, device='cuda') * 255 if i == 0 else
                 torch.randn((B, h_, w_, 64), generator=g, device='cuda'))
            idx = None
        else:
            s = 7 - i
            h_, w_ = H >> s, W >> s
            x = torch.randn((B, h_ // 2, w_ // 2, 64), generator=g, device='cuda')
            idx = torch.randint(0, 4, (B, h_ // 2, w_ // 2, 64), generator=g, device='cuda', dtype=torch.uint8)
        cp = 4 if i == 0 else 64
        wt = torch.randn((49, 64, cp), generator=g, device='cuda') * 0.01
        dy = torch.randn((B, h_, w_, 64), generator=g, device='cuda')
        f = flops[name] * B
        row = {'shape': [B, h_, w_]}
        row['fwd_ms'] = event_ms(lambda: fwd(x, wt, idx, segnet.MEAN, segnet.STD), a.iters)
        if i > 0:
            row['dgrad_ms'] = event_ms(lambda: dgrad(dy, wt, idx), a.iters)
        row['wgrad_ms'] = event_ms(lambda: wgrad(dy, x, idx, segnet.MEAN, segnet.STD), a.iters)
        for k in ('fwd', 'dgrad', 'wgrad'):
            if k + '_ms' in row:
                tf = f / (row[k + '_ms'] * 1e-3) / 1e12
                row[k + '_tflops'] = tf
                row[k + '_share_of_peak'] = tf / peak
        rows[name] = row
        del x, dy, idx
    torch.cuda.empty_cache()
    # the whole step
    tr = st.SegNetTrainer(st.init_params(0), st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy,
                          engine=eng, dtype=a.dtype, split_planes=a.split_planes)
    tr.set_group(group)
    img = torch.rand((B, 3, H, W), generator=g, device='cuda') * 255
    t = torch.randint(0, 2, (B, H, W), generator=g, device='cuda')
    tr.step(img, t)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        tr.step(img, t)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / a.iters
    kern_ms = sum(r.get(k, 0.0) for r in rows.values() for k in ('fwd_ms', 'dgrad_ms', 'wgrad_ms'))
    total_f = sum(flops.values()) * B * 3 - flops['conv1'] * B
    out = {'batch': B, 'input': [H, W], 'step_ms': step_ms, 'images_per_s': B * 1000.0 / step_ms,
           'conv_kernels_ms': kern_ms, 'conv_tflop_per_step': total_f / 1e12,
           'conv_tflops': total_f / (kern_ms * 1e-3) / 1e12, 'step_tflops': total_f / (step_ms * 1e-3) / 1e12}
    if a.split_planes:
        out.update({'split_planes': True, 'peak_tflops_f16_matrix': PEAK_TF['bf16'], 'f16_products_per_f32_product': 3,
                    'conv_share_of_peak': out['conv_tflops'] / peak, 'step_outside_conv_kernels_ms': step_ms - kern_ms})
    elif a.dtype == 'fp32':
        out['peak_tflops_f32_matrix'] = peak
    else:
        out.update({'dtype': 'bf16', 'peak_tflops_bf16_matrix': peak, 'conv_share_of_peak': out['conv_tflops'] / peak,
                    'step_outside_conv_kernels_ms': step_ms - kern_ms})
    if a.data_parallel:
        out.update({'data_parallel': True, 'world_size': group.size if group is not None else 1,
                    'backend': torch.distributed.get_backend() if group is not None else None})
    out.update({'layers': rows, 'device': torch.cuda.get_device_name(0)})
    s = json.dumps(out, indent=2)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fp:
            fp.write(s + '\n')


if __name__ == '__main__':
    main()
