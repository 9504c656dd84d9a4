#!/usr/bin/env python
"""How far the bf16 SegNet training step is from its float64 restatement without any kernel: segnet_train.reference_loss
with bf16_operands=True evaluated once in float32 and once in float64 (the same bf16 operand rounding, the same pooling
index maps), and the first MomentumSGD update (lr 0.01, weight decay 5e-4) of each compared per parameter, relative to
max |float64 update| -- the measure of tests/test_gpu_segnet_train_bf16.py and tests/test_gpu_segnet_dp.py.  Rounding to
bf16 amplifies the float32 / float64 difference of the values it rounds, so this gap is the floor for the kernels' bf16
step (init_params(5), the tests' seed-6 batch at 64 x 128).  CPU only.

  python tools/segnet_bf16_restatement_gap.py [--batch 2 4]
"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
st = importlib.import_module('superpixel-align_amd.segnet_train')


def gradients(B, dtype, maps=None, bf16=True):
    p = st.init_params(5)
    g = torch.Generator().manual_seed(6)
    img = torch.rand((B, 3, 64, 128), generator=g) * 255
    t = torch.randint(0, 2, (B, 64, 128), generator=g)
    orig = st.conv1_input
    st.conv1_input = lambda im: orig(im).to(dtype)                 # the float64 LRN input, then the tensor dtype
    try:
        P = {k: torch.tensor(p[k], dtype=dtype, requires_grad=True) for k in st.PARAM_KEYS}
        S = {k: torch.tensor(p[k], dtype=dtype) for k in st.STAT_KEYS}
        loss, pools = st.reference_loss(P, S, img.to(dtype), t, st.softmax_cross_entropy, idx_maps=maps,
                                        bf16_operands=bf16)
        grads = dict(zip(P, torch.autograd.grad(loss, list(P.values()))))
    finally:
        st.conv1_input = orig
    return {k: v.double() for k, v in grads.items()}, pools, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=[2, 4])
    a = ap.parse_args()
    for B in a.batch:
        g64, pools, p = gradients(B, torch.float64)
        g32, _, _ = gradients(B, torch.float32, maps=pools)
        errs = {}
        for k in st.PARAM_KEYS:
            decay = 0.0005 * torch.tensor(p[k], dtype=torch.float64)
            u64, u32 = -0.01 * (g64[k] + decay), -0.01 * (g32[k] + decay)
            errs[k] = float((u32 - u64).abs().max() / u64.abs().max())
        top = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
        print('B=%d: float32 vs float64 restatement of the bf16 step, worst update errors: %s'
              % (B, ', '.join('%s %.3g' % kv for kv in top)))


if __name__ == '__main__':
    main()
