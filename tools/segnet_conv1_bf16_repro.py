#!/usr/bin/env python3
"""Development aid: is the bf16 conv1 forward (spa_segnet_train_forward_bf16, Cin = 3) reproducible?  On a seeded image
and weight it runs the call --calls times per size and prints, per size, each call's SHA-256 and the number of output
values that differ from the first call's.  --save FILE keeps the first call's outputs; --ref FILE (another process,
possibly another build through SPA_LIB_PATH) also counts the values that differ from the saved ones:
    SPA_LIB_PATH=old.so python tools/segnet_conv1_bf16_repro.py --save /tmp/a.pt
    SPA_LIB_PATH=old.so python tools/segnet_conv1_bf16_repro.py --ref /tmp/a.pt ; python tools/segnet_conv1_bf16_repro.py --ref /tmp/a.pt
The float32 and split-plane forwards run beside it as controls."""
import argparse, hashlib, importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
segnet = importlib.import_module('superpixel-align_amd.segnet')
engine = importlib.import_module('superpixel-align_amd.engine')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='2x48x80,2x128x256,2x256x512,2x512x1024')
    ap.add_argument('--calls', type=int, default=4)
    ap.add_argument('--save', default=None)
    ap.add_argument('--ref', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    eng = engine.Engine(0)
    ref = torch.load(a.ref) if a.ref else {}
    keep = {}
    for size in a.sizes.split(','):
        B, H, W = (int(v) for v in size.split('x'))
        g = torch.Generator(device='cuda').manual_seed(7)
        w1 = torch.randn((49, 64, 4), generator=g, device='cuda') * 0.05
        img = torch.rand((B, 3, H, W), generator=g, device='cuda') * 255
        for mode in ('bf16', 'fp32', 'f16x3'):
            fwd = getattr(eng, 'segnet_train_forward' + {'fp32': '', 'bf16': '_bf16', 'f16x3': '_f16x3'}[mode])
            ys = [fwd(img, w1, None, segnet.MEAN, segnet.STD, stats=False)[0].clone() for _ in range(a.calls)]
            torch.cuda.synchronize()
            key = '%s %s' % (mode, size)
            row = ['%s:%d' % (hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()[:8], int((y != ys[0]).sum())) for y in ys]
            extra = ''
            if key in ref:
                extra = '  vs saved: ' + ' '.join(str(int((y.cpu() != ref[key]).sum())) for y in ys)
            print('%-22s of %9d values, sha:differing-from-call-0  %s%s' % (key, ys[0].numel(), ' '.join(row), extra), flush=True)
            if mode == 'bf16' or B * H * W <= 2 * 256 * 512:
                keep[key] = ys[0].cpu()
    if a.save:
        torch.save(keep, a.save)


if __name__ == '__main__':
    main()
