#!/usr/bin/env python
"""SegNet-Basic inference on the MI355X: per-layer device-event times of libspalign's kernels (spa_segnet_encode /
_decode / _score) at B images of 512 x 1024 (evaluated at 1024 x 2048), images/s of the whole launch chain, and each
layer's achieved TFLOP/s from the FLOPs its shape needs (segnet.layer_flops) against the matrix peak of the dtype
(PEAK_TF of tools/segnet_train_bench.py: 157.3 TF float32, 16 x that bf16).  The same layers as float32
torch.nn.functional.conv2d (MIOpen) plus separate max_pool2d / max_unpool2d on the GPU are timed as the library
baseline.  Random weights: the time does not depend on the values.

  python tools/segnet_bench.py [--dtype fp32|bf16] [--split_planes] [--compare_fp32 | --compare_all] [--batch 4]
                               [--iters 20] [--out profiles/segnet_bench.json]

--dtype bf16: the bf16 kernels (spa_segnet_encode_bf16 / _decode_bf16).  --split_planes (refused with --dtype bf16):
the float32-accurate kernels on the f16 matrix cores (spa_segnet_encode_f16x3 / _decode_f16x3), reported as mode
'f16x3' and priced against PEAK_TF['bf16'] / 3 (three f16 products per float32 product; the f16 and bf16 matrix peaks
are equal), as tools/segnet_train_bench.py prices the training passes.  --compare_fp32 (with --dtype bf16 or
--split_planes): the float32 chain is timed in the same process, the two chains alternating over --rounds rounds, and
reported under 'fp32' with the ratio of the chain times.  --compare_all: all three modes alternate round by round in
one process; the mode asked for is the top-level report, the other two follow under their names, each with its chain
ms per round and its ratio to the float32 chain.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
segnet = importlib.import_module('superpixel-align_amd.segnet')
from segnet_train_bench import PEAK_TF  # noqa: E402  (per-dtype matrix peaks, TFLOP/s)


def random_params(seed=0):
    rng = np.random.default_rng(seed)
    p = {}
    for i, name in enumerate(segnet.LAYERS):
        cin = 3 if i == 0 else 64
        p[name + '/W'] = (rng.standard_normal((64, cin, 7, 7)) * np.sqrt(2.0 / (cin * 49))).astype(np.float32)
        p[name + '_bn/gamma'] = np.ones(64, np.float32)
        p[name + '_bn/beta'] = np.full(64, 1e-3, np.float32)
        p[name + '_bn/avg_mean'] = np.zeros(64, np.float32)
        p[name + '_bn/avg_var'] = np.ones(64, np.float32)
    p['conv_classifier/W'] = (rng.standard_normal((2, 64, 1, 1)) / 8).astype(np.float32)
    p['conv_classifier/b'] = np.zeros(2, np.float32)
    return p


class LayerTimer(object):
    """model.forward(timer=...) hook: an event before each layer and at the end."""

    def __init__(self):
        self.marks = []

    def __call__(self, name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.marks.append((name, ev))

    def read(self):
        return {self.marks[i][0]: self.marks[i][1].elapsed_time(self.marks[i + 1][1]) for i in range(len(self.marks) - 1)}


def library_forward(p, x, timer):
    """float32 conv2d (MIOpen) + max_pool2d(return_indices) / max_unpool2d + classifier + softmax, BN folded."""
    F = torch.nn.functional
    f = segnet.fold_bn(p)
    w = {k: (torch.from_numpy(v[0]).cuda(), torch.from_numpy(v[1]).cuda()) for k, v in f.items()}
    h = x.clone()
    for c in range(3):
        h[:, c] = (h[:, c] - float(segnet.MEAN[c])) / float(segnet.STD[c])
    h = h * (1.0 + 1e-4 / 5 * (h * h).sum(1, keepdim=True)) ** -0.75
    idxs = []
    for name in segnet.ENCODERS:
        timer(name)
        h, i = F.max_pool2d(torch.relu(F.conv2d(h, w[name][0], w[name][1], padding=3)), 2, 2, return_indices=True)
        idxs.append(i)
    for name, i in zip(segnet.DECODERS, idxs[::-1]):
        timer(name)
        h = F.conv2d(F.max_unpool2d(h, i, 2, 2), w[name][0], w[name][1], padding=3)
    z = F.conv2d(h, w['conv_classifier'][0][:, :, None, None], w['conv_classifier'][1])
    timer(None)
    return torch.softmax(z, 1)


def timed(fn, iters):
    per = []
    for _ in range(iters):
        t = LayerTimer()
        fn(t)
        torch.cuda.synchronize()
        per.append(t.read())
    return {k: float(np.median([d[k] for d in per])) for k in per[0]}


def chain_ms(chain, iters):
    """ms per chain: events around whole chains, no per-layer events inside"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        chain()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


MODES = ('fp32', 'bf16', 'f16x3')
MODE_PEAK = {'fp32': PEAK_TF['fp32'], 'bf16': PEAK_TF['bf16'], 'f16x3': PEAK_TF['bf16'] / 3}
MODE_NAME = {'fp32': 'float32', 'bf16': 'bf16', 'f16x3': 'split-plane f16 (float32-accurate)'}


def report(mode, a, layers, ms, flops):
    peak = MODE_PEAK[mode]
    res = {'what': 'SegNet-Basic inference, libspalign %s MFMA kernels' % MODE_NAME[mode],
           'dtype': 'bf16' if mode == 'bf16' else 'fp32', 'split_planes': mode == 'f16x3', 'batch': a.batch, 'input': [a.H, a.W], 'eval_shape': [2 * a.H, 2 * a.W], 'iters': a.iters,
           'chain_ms': ms, 'images_per_s': a.batch * 1000.0 / ms, 'peak_tflops_matrix': peak, 'layers': {}}
    res['network_tflops'] = sum(flops.values()) / (ms * 1e-3) / 1e12
    res['network_share_of_peak'] = res['network_tflops'] / peak
    for k, t in layers.items():
        row = {'ms': t}
        if k in flops:
            tf = flops[k] / (t * 1e-3) / 1e12
            row.update(gflop=flops[k] / 1e9, tflops=tf, share_of_peak=tf / peak)
        res['layers'][k] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--split_planes', action='store_true', help='the float32-accurate kernels on the f16 matrix cores')
    ap.add_argument('--compare_fp32', action='store_true',
                    help='with --dtype bf16 or --split_planes: time the float32 chain too')
    ap.add_argument('--compare_all', action='store_true', help='alternate the fp32, bf16 and split-plane chains')
    ap.add_argument('--rounds', type=int, default=3, help='alternations of the chains under --compare_fp32 / _all')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--H', type=int, default=512)
    ap.add_argument('--W', type=int, default=1024)
    ap.add_argument('--no_library', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    if a.split_planes and a.dtype != 'fp32':
        ap.error('--split_planes is the float32-accurate mode: it cannot be combined with --dtype %s' % a.dtype)
    if not torch.cuda.is_available():
        raise SystemExit('segnet_bench: no GPU (nothing is measured without one)')
    torch.cuda.set_device(0)
    p = random_params()
    main_mode = 'f16x3' if a.split_planes else a.dtype
    if a.compare_all:
        dtypes = [main_mode] + [m for m in MODES if m != main_mode]
    else:
        dtypes = [main_mode] + (['fp32'] if a.compare_fp32 and main_mode != 'fp32' else [])
    models = {m: segnet.SegNetBasic(p, pred_shape=(2 * a.H, 2 * a.W), dtype='bf16' if m == 'bf16' else 'fp32',
                                    split_planes=m == 'f16x3') for m in dtypes}
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randint(0, 256, (a.batch, 3, a.H, a.W), generator=g, device='cuda').float()
    flops = {k: v * a.batch * (a.H * a.W) / (512.0 * 1024.0) for k, v in segnet.layer_flops().items()}

    def chain_of(model):
        def chain(t=None):
            prob = model.forward(x, timer=t)
            if t is not None:
                t('score')
            model.engine.segnet_score(prob, (2 * a.H, 2 * a.W))
            if t is not None:
                t(None)
        return chain

    chains = {dt: chain_of(m) for dt, m in models.items()}
    for dt in dtypes:
        for _ in range(a.warmup):
            chains[dt]()
    torch.cuda.synchronize()
    per_layer = {dt: [] for dt in dtypes}
    per_chain = {dt: [] for dt in dtypes}
    for _ in range(a.rounds if len(dtypes) > 1 else 1):
        for dt in dtypes:
            per_layer[dt].append(timed(chains[dt], a.iters))
            per_chain[dt].append(chain_ms(chains[dt], a.iters))
    out = {}
    for dt in dtypes:
        layers = {k: float(np.median([d[k] for d in per_layer[dt]])) for k in per_layer[dt][0]}
        out[dt] = report(dt, a, layers, float(np.median(per_chain[dt])), flops)
    res = out[main_mode]
    if main_mode == 'fp32':
        res['peak_tflops_f32_matrix'] = PEAK_TF['fp32']
    if len(dtypes) > 1:
        res['rounds'] = a.rounds
        for dt in dtypes:
            out[dt]['chain_ms_rounds'] = per_chain[dt]
            if dt != 'fp32':
                out[dt]['chain_ratio_to_fp32'] = out[dt]['chain_ms'] / out['fp32']['chain_ms']
                out[dt]['chain_ratio_to_fp32_rounds'] = [m / f for m, f in zip(per_chain[dt], per_chain['fp32'])]
            if dt != main_mode:
                res[dt] = out[dt]
    if not a.no_library:
        for _ in range(a.warmup):
            library_forward(p, x, lambda n: None)
        torch.cuda.synchronize()
        lib = timed(lambda t: library_forward(p, x, t), a.iters)
        res['library'] = {k: {'ms': ms, 'tflops': flops[k] / (ms * 1e-3) / 1e12} for k, ms in lib.items()}
        res['library_network_ms'] = sum(lib.values())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
