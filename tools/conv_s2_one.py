"""The stride-2 openers alone (spa_conv3x3_s2_f16s): the generic kernel (Engine.debug_set(3, 0)) and the 2-D tile kernel (3, 1) timed in
one process, with a digest of y, y2 and the tracked maximum of each, the error against float64 and MIOpen + epilogue passes for scale.
    python tools/conv_s2_one.py [--reps 5] [--launches 10]
Per shape: `reps` repetitions per kernel, alternating, each the mean of `launches` back-to-back launches between two events."""
import argparse, hashlib, importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, torch.nn.functional as F

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--launches', type=int, default=10)
ap.add_argument('--bench-only', action='store_true', help='the two 30-image shapes of bench.py only')
args = ap.parse_args()
eng = importlib.import_module('superpixel-align_amd.engine').Engine()
torch.manual_seed(3)


def digest(*ts):
    h = hashlib.sha1()
    for t in ts:
        h.update(t.contiguous().view(torch.int32).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def timed(fn, n):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n


SHAPES = ((32, 64, 512, 1024, 30), (64, 128, 256, 512, 30), (32, 64, 37, 301, 2), (64, 128, 20, 270, 1))
for (C, K, Hi, Wi, B) in (SHAPES[:2] if args.bench_only else SHAPES):
    x = (torch.relu(torch.randn((B, C, Hi, Wi), device='cuda')) * 2.3).contiguous(memory_format=torch.channels_last)
    w = torch.randn((K, C, 3, 3), device='cuda') * (2.0 / (9 * C)) ** 0.5
    wd = torch.randn((K, C, 1, 1), device='cuda') * (2.0 / C) ** 0.5
    b = torch.randn((2 * K,), device='cuda')
    wc = torch.zeros((2 * K, 9, C), device='cuda')
    wc[:K] = w.permute(0, 2, 3, 1).reshape(K, 9, C); wc[K:, 4] = wd.reshape(K, C)
    wt2, inv_t = eng.split_planes(wc)
    am_in = eng.amax(x)
    nb = min(B, 2)
    r1 = torch.relu(F.conv2d(x[:nb].double(), w.double(), b[:K].double(), 2, 1))
    r2 = F.conv2d(x[:nb].double(), wd.double(), b[K:].double(), 2, 0)
    Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
    gb = B * (Hi * Wi * C + 2 * Ho * Wo * K) * 4 / 1e9          # the input once, both outputs once
    print('%d->%d+%d %dx%d B%d (%.2f GB in + y + y2)' % (C, K, K, Hi, Wi, B, gb))
    times = {0: [], 1: []}
    for rep in range(args.reps):
        for key in (0, 1):
            eng.debug_set(3, key)
            times[key].append(timed(lambda: eng.conv3x3_s2_f16s(x, wt2, inv_t, b, K, True, amax_in=am_in), args.launches))
    for key, name in ((0, 'generic kernel  '), (1, '2-D tile kernel ')):
        eng.debug_set(3, key)
        y, y2, am = eng.conv3x3_s2_f16s(x, wt2, inv_t, b, K, True, amax_in=am_in)
        t = times[key]
        print('  %s %s ms  min %.3f (%.2f TB/s)  spread %.3f   conv %.2e  projection %.2e of scale vs float64; amax %.6g (torch %.6g); digest %s' % (
            name, ' '.join('%.3f' % v for v in t), min(t), gb / min(t), max(t) - min(t),
            (y[:nb].double() - r1).abs().max().item() / r1.abs().max().item(), (y2[:nb].double() - r2).abs().max().item() / r2.abs().max().item(),
            am.view(torch.float32).item(), y.abs().max().item(), digest(y, y2, am)))
    eng.debug_set(3, 1)

    def mi():
        a = F.conv2d(x, w, None, 2, 1); eng.bias_act_(a, b[:K].contiguous(), None, True)
        c = F.conv2d(x, wd, None, 2, 0); eng.bias_act_(c, b[K:].contiguous(), None, False)
    print('  MIOpen + epilogues %.3f ms' % timed(mi, 3))
