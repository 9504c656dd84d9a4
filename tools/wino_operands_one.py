"""The three kernels of a split-plane Winograd layer (spa_conv3x3_wino4_f16s: k_wino4_in, the GEMM, k_wino4_out_s) timed alone for the
operand paths of Engine.debug_set(4, v): 0 = sub-grid-major tile numbering and float32 V, 1 = the sub-grids of a pixel row interleaved
(dilation > 2), 2 = that numbering and V written as the GEMM's planes (Cout from 512 on).  30 images of a 128 x 256 map, the layers of DRN-D-22 plus the dilation-1 control.
    python tools/wino_operands_one.py [--reps 5] [--launches 10]
Per shape: one round over the paths that is not counted, then `reps` repetitions per path, alternating, each the mean of `launches` launches (the library's per-kernel
events); per kernel the minimum and the spread (max - min) of the repetitions, and a digest of y and the tracked maximum (the same for
all three)."""
import argparse, hashlib, importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--launches', type=int, default=10)
ap.add_argument('--images', type=int, default=30)
ap.add_argument('--keys', default='0,1,2')
args = ap.parse_args()
eng = importlib.import_module('superpixel-align_amd.engine').Engine()
torch.manual_seed(3)
KEYS = tuple(int(k) for k in args.keys.split(','))


def digest(*ts):
    h = hashlib.sha1()
    for t in ts:
        h.update(t.contiguous().view(torch.int32).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def part(name):
    return 'in' if name == 'k_wino_in' else ('out' if name == 'k_wino_out' else 'gemm')


B, H, W = args.images, 128, 256
for (C, K, d) in ((512, 512, 1), (512, 512, 2), (512, 512, 4), (256, 512, 4), (256, 256, 2)):
    x = (torch.relu(torch.randn((B, C, H, W), device='cuda')) * 2.3).contiguous(memory_format=torch.channels_last)
    w = torch.randn((K, C, 3, 3), device='cuda') * (2.0 / (9 * C)) ** 0.5
    b = torch.randn((K,), device='cuda')
    res = torch.randn((B, K, H, W), device='cuda').contiguous(memory_format=torch.channels_last)
    u2, cs = eng.winograd_weights_split(w)
    am = eng.amax(x)
    y = torch.empty_like(res)
    T = int(eng._lib.spa_wino4_tiles(B, H, W, d))
    scratch = (torch.empty((36, T, C), device='cuda'), torch.empty((36, T, K), device='cuda'))
    run = lambda: eng.conv3x3_wino_f16s(x, u2, cs, b, res, True, d, amax_in=am, out=y, scratch=scratch)
    print('%d->%d d=%d B%d %dx%d' % (C, K, d, B, H, W), flush=True)
    times = {k: {'in': [], 'gemm': [], 'out': []} for k in KEYS}
    digests = {}
    for rep in range(-1, args.reps):
        for key in KEYS:
            eng.debug_set(4, key)
            run(); torch.cuda.synchronize()
            eng.prof_enable(True)
            for _ in range(args.launches): run()
            for name, (ms, n) in eng.prof_read().items():
                if rep >= 0: times[key][part(name)].append(ms / n)
            eng.prof_enable(False)
            if rep == 0:
                yy, a = run()
                digests[key] = digest(yy, a)
    for key in KEYS:
        print('  key4=%d  digest %s' % (key, digests[key]))
        for p in ('in', 'gemm', 'out'):
            t = times[key][p]
            print('    %-5s %s ms  min %.3f  spread %.3f' % (p, ' '.join('%.3f' % v for v in t), min(t), max(t) - min(t)), flush=True)
    eng.debug_set(4, 2)
    del x, w, res, y, scratch
