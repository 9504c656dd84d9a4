#!/usr/bin/env python
"""SegNet-Basic inference on the MI355X: per-layer device-event times of libspalign's kernels (spa_segnet_encode /
_decode / _score) at B images of 512 x 1024 (evaluated at 1024 x 2048), images/s of the whole launch chain, and each
layer's achieved TFLOP/s from the FLOPs its shape needs (segnet.layer_flops) against the 157.3 TF float32 matrix peak.
The same layers as float32 torch.nn.functional.conv2d (MIOpen) plus separate max_pool2d / max_unpool2d on the GPU are
timed as the library baseline.  Random weights: the time does not depend on the values.

  python tools/segnet_bench.py [--batch 4] [--iters 20] [--out profiles/segnet_bench.json]
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
segnet = importlib.import_module('superpixel-align_amd.segnet')
PEAK_TF = 157.3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--H', type=int, default=512)
    ap.add_argument('--W', type=int, default=1024)
    ap.add_argument('--no_library', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('segnet_bench: no GPU (nothing is measured without one)')
    torch.cuda.set_device(0)
    p = random_params()
    model = segnet.SegNetBasic(p, pred_shape=(2 * a.H, 2 * a.W))
    eng = model.engine
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randint(0, 256, (a.batch, 3, a.H, a.W), generator=g, device='cuda').float()
    flops = {k: v * a.batch * (a.H * a.W) / (512.0 * 1024.0) for k, v in segnet.layer_flops().items()}

    def chain(t=None):
        prob = model.forward(x, timer=t)
        if t is not None:
            t('score')
        eng.segnet_score(prob, (2 * a.H, 2 * a.W))
        if t is not None:
            t(None)

    for _ in range(a.warmup):
        chain()
    torch.cuda.synchronize()
    layers = timed(chain, a.iters)
    # end to end: events around whole chains, no per-layer events inside
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.iters):
        chain()
    e.record()
    torch.cuda.synchronize()
    chain_ms = s.elapsed_time(e) / a.iters
    res = {'what': 'SegNet-Basic inference, libspalign float32 MFMA kernels', 'batch': a.batch, 'input': [a.H, a.W],
           'eval_shape': [2 * a.H, 2 * a.W], 'iters': a.iters, 'chain_ms': chain_ms,
           'images_per_s': a.batch * 1000.0 / chain_ms, 'peak_tflops_f32_matrix': PEAK_TF, 'layers': {}}
    total_flop = sum(flops.values())
    res['network_tflops'] = total_flop / (chain_ms * 1e-3) / 1e12
    for k, ms in layers.items():
        row = {'ms': ms}
        if k in flops:
            tf = flops[k] / (ms * 1e-3) / 1e12
            row.update(gflop=flops[k] / 1e9, tflops=tf, share_of_peak=tf / PEAK_TF)
        res['layers'][k] = row
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
