"""Inputs on which the felzenszwalb kernels are most likely to go wrong, as one table that the CPU test
(test_fz_cases_cpu.py: the cases themselves, against a plain sequential reference) and the GPU test
(test_gpu_felzenszwalb_hostile.py: the kernels, against the oracle) share.  Numpy only.

The shapes bracket the switch of fz_run (csrc/spa_felz.hip) between k_fz_pass_tab<true> (parent array
in LDS) and k_fz_pass_tab<false> (parent array in global memory, hub chains): see lpar() below."""
import collections

import numpy as np


# ------------------------------------------------------------------------------------------ generators
def noise(seed, H, W, lo=0, hi=256):
    """iid integers in [lo, hi) per channel and pixel; (3, H, W) float32."""
    return np.random.RandomState(seed).randint(lo, hi, size=(3, H, W)).astype(np.float32)


def checker(H, W, period):
    """Two-valued checkerboard with squares of `period` pixels."""
    ys, xs = np.mgrid[0:H, 0:W]
    on = ((ys // period + xs // period) & 1).astype(np.float32)
    return np.stack([40 + 160 * on, 200 - 150 * on, 10 + 90 * on]).astype(np.float32)


def stripes(H, W, width):
    """Vertical stripes of `width` pixels; the stripe values differ per channel."""
    k = (np.arange(W) // width).astype(np.int64)
    row = np.stack([(k * 37) % 256, (k * 91 + 50) % 256, (k * 53 + 120) % 256]).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(row[:, None, :], (3, H, W)))


def constant(H, W, v):
    return np.full((3, H, W), v, np.float32)


GENERATORS = {'noise': noise, 'checker': checker, 'stripes': stripes, 'constant': constant}


# ------------------------------------------------------------------------------------------ the kernel switch
# fz_run, csrc/spa_felz.hip, the lines "const size_t lds_limit = 156 * 1024;" to "if (cells > 4096) cells = 4096;":
#   par_bytes = (npix * 2 + 15) & ~15;  lpar = npix <= 65535 && par_bytes + 2560 * 16 + FZ_THREADS * 4 <= lds_limit;
#   cells = lpar ? (lds_limit - par_bytes - FZ_THREADS * 4) / 16 : 4096, at most 4096          (FZ_THREADS = 1024)
LDS_LIMIT = 156 * 1024
MIN_CELLS = 2560
LPAR_MAX_NPIX = 57344


def par_bytes(npix):
    return (2 * npix + 15) & ~15


def lpar(npix):
    return npix <= 65535 and par_bytes(npix) + MIN_CELLS * 16 + 4096 <= LDS_LIMIT


def cells(npix):
    return min(4096, (LDS_LIMIT - par_bytes(npix) - 4096) // 16) if lpar(npix) else 4096


# ------------------------------------------------------------------------------------------ the cases
# gen: (generator name, arguments without H and W in front — 'synth_image' / 'synth_scene' are the package's, (seed,)).
# forms: 'f32' (spa_felzenszwalb) or 'both' (also spa_felzenszwalb_u8 on the image truncated to 8 bits: / 255 in
#        float64) — 'both' exactly where the two forms give different labels.
# batch: images in the GPU call; image i of a seeded generator takes seed + i (unseeded ones repeat).
# prop:  what the case claims of the oracle's result (checked in test_fz_cases_cpu.py):
#        n == / n >= number of segments, smallest / largest segment, sizes (sorted), zero_cost (every edge),
#        max_costs (distinct non-zero edge costs of the 8-bit form at most), tie_group_min (non-zero costs per distinct
#        one, more than), cleanup_majority (more than half of all unions in pass 2).
Case = collections.namedtuple('Case', 'name gen H W scale sigma min_size forms batch prop')


def _c(name, gen, H, W, scale, sigma, min_size, forms='f32', batch=1, **prop):
    return Case(name, gen, H, W, float(scale), float(sigma), int(min_size), forms, batch, prop)


CASES = [
    # white noise: pass 0 merges little, the clean-up pass does most of the merging in long dependent chains
    _c('noise_224x256', ('noise', 1), 224, 256, 300, 0.8, 20, batch=4, n_min=50, smallest=20),     # 57 344: last LPAR size
    _c('noise_143x401', ('noise', 2), 143, 401, 300, 0.8, 20, batch=3),                            # 57 343, rounded up
    _c('noise_15x3823', ('noise', 3), 15, 3823, 300, 0.8, 20, batch=3),                            # 57 345: first !LPAR
    _c('noise_239x240_r0', ('noise', 4), 239, 240, 300, 0.1, 20, batch=3),                         # 57 360, radius 0
    _c('noise300_64x96', ('noise', 5), 64, 96, 300, 0.8, 20, n_min=5),
    # ... at scale 300 that is not so (64x96: 6 013 unions in pass 0, 118 in the clean-up pass); at scale 3 it is (5 and 6 040)
    _c('noise_64x96', ('noise', 5), 64, 96, 3, 0.8, 20, n_min=50, cleanup_majority=True),
    _c('cleanup_224x256', ('noise', 18), 224, 256, 3, 0.8, 20, n_min=50, smallest=20),
    _c('cleanup_239x240', ('noise', 19), 239, 240, 3, 0.8, 20, n_min=50, smallest=20),
    # few-valued noise, radius 0: tie groups of thousands of equal costs over the four edge families.  The 8-bit form has
    # 18 distinct non-zero costs; the float32 form 55, because x / 255 rounded to float32 splits equal differences
    _c('few_224x256', ('noise', 6, 0, 4), 224, 256, 30, 0.1, 20, forms='both', batch=3, max_costs=40, tie_group_min=5000),
    _c('few_240x241', ('noise', 7, 0, 4), 240, 241, 30, 0.1, 20, forms='both', batch=3, max_costs=40, tie_group_min=5000),
    _c('few_64x96', ('noise', 8, 0, 4), 64, 96, 30, 0.1, 20, forms='both', max_costs=40),
    # k = scale / 255 a hair beside the cost 1 / 255 of a one-step difference: the float32 rounding of the threshold
    # decides whether single pixels merge over such an edge (min_size 1: the clean-up pass hides nothing)
    _c('few_k_above_48x64', ('noise', 20, 0, 4), 48, 64, 1 + 1e-9, 0.1, 1, forms='both'),
    _c('few_k_below_48x64', ('noise', 20, 0, 4), 48, 64, 1 - 1e-9, 0.1, 1),
    # two values: one tie group of zero costs and one of the single non-zero cost
    _c('checker1_224x256', ('checker', 1), 224, 256, 300, 0.1, 20, batch=3, n=2, sizes=(28672, 28672)),
    _c('checker1_64x96', ('checker', 1), 64, 96, 300, 0.1, 20, n=2, sizes=(3072, 3072)),
    _c('checker3_61x95', ('checker', 3), 61, 95, 300, 0.8, 4),
    _c('stripes7_239x240', ('stripes', 7), 239, 240, 300, 0.1, 20, n=35),
    _c('stripes5_64x96', ('stripes', 5), 64, 96, 300, 0.8, 20),
    # degenerate ends
    _c('constant_239x240', ('constant', 77.0), 239, 240, 300, 0.8, 20, n=1, zero_cost=True),
    _c('constant_16x24', ('constant', 0.0), 16, 24, 300, 0.1, 20, n=1, zero_cost=True),
    _c('nomerge_96x128', ('noise', 9), 96, 128, 1e-3, 0.1, 1, n=96 * 128),                         # every pixel a root
    _c('allmerge_48x64', ('noise', 10), 48, 64, 300, 0.8, 5000, n=1),                              # min_size > npix
    _c('noise_2x2_nomerge', ('noise', 11), 2, 2, 1e-3, 0.1, 1, n=4),
    _c('noise_2x2_onemerge', ('noise', 12), 2, 2, 300, 0.8, 20, n=1),
    # hub chains (!LPAR): one giant component absorbs small ones
    _c('hub_239x240', ('synth_image', 3), 239, 240, 30, 0.8, 20, forms='both', n_min=20, largest_min=239 * 240 // 3 + 1),
    # radius 31, the largest both sides accept; larger than the 5x9 image, whose reflection wraps several periods.
    # scale 300 leaves one segment on both; scale 0.5 / min_size 1 chosen on the CPU: 177 and 7 segments
    _c('r31_40x56', ('noise', 13), 40, 56, 0.5, 7.8, 1, n_min=2),
    _c('r31_5x9', ('noise', 14), 5, 9, 0.5, 7.8, 1, n_min=2),
    _c('r12_3x5', ('noise', 15), 3, 5, 0.5, 3.0, 1),
    # the existing families at small sizes
    _c('scene_48x64', ('synth_scene', 16), 48, 64, 300, 0.8, 20),
    _c('image_64x96', ('synth_image', 17), 64, 96, 30, 0.8, 20, forms='both'),
]
BY_NAME = {c.name: c for c in CASES}
SMALL = [c for c in CASES if c.H * c.W <= 64 * 96]


def image(case, synth, i=0, uint8_image=False):
    """Image i of the case's batch; `synth` is the package's synth module (the conftest fixture)."""
    if uint8_image:
        return image(case, synth, i).astype(np.uint8)
    kind, args = case.gen[0], case.gen[1:]
    if kind == 'synth_image':
        return synth.synth_image(args[0] + i, case.H, case.W)
    if kind == 'synth_scene':
        return synth.synth_scene(args[0] + i, case.H, case.W, n_rect=12)
    if kind == 'noise':
        return noise(args[0] + 1000 * i, case.H, case.W, *args[1:])
    return GENERATORS[kind](case.H, case.W, *args)


def batch(case, synth, uint8_image=False):
    return np.stack([image(case, synth, i, uint8_image) for i in range(case.batch)])
