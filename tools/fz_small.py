#!/usr/bin/env python3
"""Development aid: felzenszwalb time at the reference operating point (30 images of 224x224)."""
import importlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
spa = importlib.import_module('superpixel-align_amd')
eng = importlib.import_module('superpixel-align_amd.engine').default_engine()
x = torch.from_numpy(np.stack([spa.synth.synth_scene(s, 224, 224) for s in range(30)])).cuda()
eng.felzenszwalb(x, 300.0, 0.8, 20); torch.cuda.synchronize()
t = time.time()
for _ in range(5):
    lab, nl = eng.felzenszwalb(x, 300.0, 0.8, 20)
torch.cuda.synchronize()
print('felzenszwalb 30 x 224x224: %.2f ms per batch; segments %s' % ((time.time() - t) / 5 * 1e3, nl[:4].tolist()))
# pass diagnostics of the last call (k_fz_pass_tab): windows, chunks, rounds summed over images and both passes;
# WS_CONNMISC holds zcount[256], then the 16 diagnostic words
import ctypes, re
lib_mod = importlib.import_module('superpixel-align_amd._lib')
src = open(os.path.join(os.path.dirname(lib_mod.__file__), 'csrc', 'spa_common.h')).read()
names = re.findall(r'^\s*(WS_[A-Z_0-9]+)\s*(?:=\s*0)?,', src, re.M)
host = (ctypes.c_int32 * 9)()
lib_mod.check(lib_mod.lib().spa_debug_peek(eng._ctx, names.index('WS_CONNMISC'), 256 * 4, 36, host))
print('per image and both passes: %.0f windows, %.0f chunks of 1024 sorted edges, %.0f full rounds, %.0f tail rounds' % tuple(v / 30.0 for v in host[:4]))
print('kilo-cycles per image: flatten %.0f | collect %.0f | window set-up + write-back %.0f | full rounds %.0f | tail %.0f' % tuple(v / 30.0 for v in host[4:9]))
