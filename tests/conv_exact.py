"""Operands on which the direct MFMA convolutions have ONE right answer, bit for bit, the reference that gives it and the check.

The tolerance tests of the DRN convolutions (test_gpu_conv.py, test_gpu_pipeline.py) bound the largest error by a fraction of the
largest output.  Once K = 9 Cin is large, a typical term of the sum is smaller than that bound, and the references of the bf16 forms
are float32 convolutions run on the same GPU.  Here the operands are small integers, so

  * every product and every partial sum of an output is an integer multiple of one unit u (u = 1 for the bf16 and float32 forms;
    u = sc t for the split-plane forms, whose scales sc = 2^(14 - e) of the pixels and t of the weights are powers of two),
  * every one of them is below 2^24 u in magnitude (`Case.bound`, asserted when the operands are made),

and a float32 accumulator holds each of them exactly IN ANY ORDER of summation.  The output is then the exact sum, through the
epilogue's exact power-of-two unscale, bias, residual and ReLU, rounded once to the output type: float32 holds it as it is, bf16
rounds it to nearest even.  A dropped, doubled or misplaced term changes an integer by at least 1, so `check` is torch.equal: no
tolerance, no exempt element.

PREMISE.  A matrix instruction (v_mfma_f32_16x16x32_bf16 / _f16, v_mfma_f32_16x16x16_bf16, v_mfma_f32_16x16x4_f32) loses no bit of
a sum whose every addend and every partial sum is representable in 24 significand bits of one common unit.  That holds for any
adder that aligns its addends to the largest exponent and keeps 24 bits, truncating or rounding; nobody has measured it on gfx950
for this project.  A kernel that differs on these operands is a finding to trace in the kernel or in this premise (DESIGN.md
section 7 records the outcome); it is never a reason to add a tolerance.

Regimes (bias and residual are integers in [-8, 8] in all of them):
    'unit'      x, w in {-1, +1}.  |sum| stays below 256 (asserted on the REFERENCE for 99 % of the outputs, `unit_fraction`), where
                bf16 holds every integer: a change of one output by 1 shows in the bf16 result.
    'wide'      x in 0..7, w in -3..3.  Outputs reach ~2000 with both signs in front of the ReLU, so the bf16 forms round, and
                10-20 % of the outputs are exact ties of that rounding.
    'planes_x'  (split-plane forms) x an odd-heavy signed integer up to 4095: after the power-of-two scale its 12 bits need a
                non-zero low half-precision plane; w a small integer whose low plane is zero.
    'planes_w'  the other way round.  The kernels drop the product of the two low planes by design, so only ONE operand may carry
                one; the small operand's magnitude is chosen per K so that the bound holds.

The reference is torch's float64 convolution on the CPU (exact on these integers in any order: every sum is below 2^53), cast to
float32 (exact, asserted) and from there to the output type.  Nothing here touches a GPU.
"""
import functools

import torch

F = torch.nn.functional

REGIMES = ('unit', 'wide', 'planes_x', 'planes_w')
BR_MAX = 8                   # |bias|, |residual| <= 8
BIG = 4095                   # the operand that needs the low plane
LIMIT = 1 << 24


def split(t):
    """The two half-precision planes of a float tensor as the kernels and Engine.split_planes make them: s = 2^(14 - e) with e the
    exponent of the largest magnitude, h = rn16(s t), l = rn16(s t - h).  -> (h, l, s), h and l float32 holding half values."""
    amax = float(t.abs().max())
    e = 0 if amax == 0.0 else int(torch.floor(torch.log2(torch.tensor(amax, dtype=torch.float64))))
    s = 2.0 ** (14 - e)
    ts = (t.double() * s).float()
    assert torch.equal(ts.double(), t.double() * s)                           # a power of two: exact
    h = ts.half().float()
    l = (ts - h).half().float()
    return h, l, s


class Case:
    """One convolution with exact operands.  x (B,Cin,H,W), w (Cout,Cin,k,k), bias (Cout), res (B,Cout,Ho,Wo) or None and, for the
    opener + projection forms, wd (Cp,Cin,1,1) and bias2 (Cp): float64 CPU tensors holding integers."""

    def __init__(self, regime, B, Cin, Cout, H, W, taps=9, stride=1, dil=1, res=False, relu=True, proj=0, seed=0):
        assert regime in REGIMES and taps in (1, 9) and stride in (1, 2)
        self.regime, self.taps, self.stride, self.dil, self.relu, self.proj = regime, taps, stride, dil, relu, proj
        k = 3 if taps == 9 else 1
        self.K = taps * Cin
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * Cin + 31 * Cout + 17 * H + W + taps + len(regime))
        Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
        xs, ws, ds = (B, Cin, H, W), (Cout, Cin, k, k), (proj, Cin, 1, 1)

        def ints(shape, lo, hi):
            return torch.randint(lo, hi + 1, shape, generator=g).double()

        def big(shape):
            v = torch.randint(0, BIG + 1, shape, generator=g)
            v = torch.where(torch.rand(shape, generator=g) < 0.75, v | 1, v)          # odd-heavy: the lowest bit is in use
            v = (v * (2 * torch.randint(0, 2, shape, generator=g) - 1)).double()
            v.view(-1)[0] = BIG                                                       # the scale is that of 4095 whatever the draw
            return v

        # the small operand of the plane regimes: as large as the bound allows for this K, 7 at most (4097 = |h| + |l| of 4095)
        m = min(7, (LIMIT - 1 - 2 * BR_MAX) // ((BIG + 2) * self.K))
        if regime == 'unit':
            self.x, self.w = 2 * ints(xs, 0, 1) - 1, 2 * ints(ws, 0, 1) - 1
            self.wd = 2 * ints(ds, 0, 1) - 1 if proj else None
        elif regime == 'wide':
            self.x, self.w = ints(xs, 0, 7), ints(ws, -3, 3)
            self.wd = ints(ds, -3, 3) if proj else None
        elif regime == 'planes_x':
            assert m >= 1
            self.x, self.w = big(xs), ints(ws, -m, m)
            self.wd = ints(ds, -m, m) if proj else None
        else:
            assert m >= 1
            self.x, self.w = ints(xs, -m, m), big(ws)
            self.wd = big(ds) if proj else None
        self.bias = ints((Cout,), -BR_MAX, BR_MAX)
        self.bias2 = ints((proj,), -BR_MAX, BR_MAX) if proj else None
        self.res = ints((B, Cout, Ho, Wo), -BR_MAX, BR_MAX) if res else None
        self._refs = {}
        self._assert_bound()

    def _assert_bound(self):
        """every product and partial sum below 2^24 units, in ANY order: the sum of the magnitudes of all addends is"""
        def reach(t):                                   # the largest |h| + |l| of a split operand, in the operand's own units
            h, l, s = split(t)
            return float((h.abs() + l.abs()).max()) / s
        wmax = self.w.abs().max() if self.wd is None else max(self.w.abs().max(), self.wd.abs().max())
        if self.regime.startswith('planes'):
            bigt, small = (self.x, self.w) if self.regime == 'planes_x' else (self.w, self.x)
            for t in [small] + ([self.wd] if self.wd is not None and self.regime == 'planes_x' else []):
                assert not bool(split(t)[1].any()), 'the small operand must not carry a low plane'
            assert bool(split(bigt)[1].any()), 'the big operand must carry a low plane'
            xm = reach(self.x)
            wm = reach(self.w if self.wd is None else torch.cat([self.w.reshape(-1), self.wd.reshape(-1)]))
        else:
            xm, wm = float(self.x.abs().max()), float(wmax)
        self.bound = xm * wm * self.K + BR_MAX + (BR_MAX if self.res is not None else 0)
        assert self.bound < LIMIT, (self.regime, self.K, self.bound)

    # ------------------------------------------------------------------ the reference
    def ref64(self):
        """(y, y2 or None) in float64: the exact integers"""
        if 64 not in self._refs:
            pad = self.dil if self.taps == 9 else 0
            y = F.conv2d(self.x, self.w, self.bias, self.stride, pad, self.dil)
            if self.res is not None:
                y = y + self.res
            if self.relu:
                y = torch.relu(y)
            y2 = F.conv2d(self.x, self.wd, self.bias2, self.stride, 0) if self.proj else None
            for t in (y, y2):
                assert t is None or float(t.abs().max()) < LIMIT
            self._refs[64] = (y, y2)
            if self.regime == 'unit':                   # the condition of the regime, on the reference, never on a kernel's output
                assert self.unit_fraction() >= 0.99, (self.K, self.unit_fraction())
        return self._refs[64]

    def ref(self, dtype):
        """(y, y2 or None) of the output type: float64 -> float32 is exact here, then one rounding (to nearest even) to bf16"""
        if dtype not in self._refs:
            out = []
            for t in self.ref64():
                if t is None:
                    out.append(None)
                    continue
                t32 = t.float()
                assert torch.equal(t32.double(), t)
                out.append(t32.to(dtype))
            self._refs[dtype] = tuple(out)
        return self._refs[dtype]

    def unit_fraction(self):
        """share of the reference's outputs a change by 1 is visible at in bf16"""
        return float((self.ref64()[0].abs() <= 256).double().mean())

    def wt(self):
        """the weights as the kernels take them: (Cout, taps, Cin), tap = ky * 3 + kx"""
        return self.w.permute(0, 2, 3, 1).reshape(self.w.shape[0], self.taps, self.w.shape[1]).contiguous()

    def wt_proj(self):
        """(Cout + Cp, 9, Cin): the projection's rows hold its weights at the centre tap (spa_conv3x3_s2_f16s / _f32)"""
        Cout, Cin = self.w.shape[0], self.w.shape[1]
        wc = torch.zeros((Cout + self.proj, 9, Cin), dtype=torch.float64)
        wc[:Cout] = self.wt()
        wc[Cout:, 4] = self.wd.reshape(self.proj, Cin)
        return wc

    def bias_all(self):
        return self.bias if not self.proj else torch.cat([self.bias, self.bias2])


@functools.lru_cache(maxsize=None)
def case(regime, B, Cin, Cout, H, W, taps=9, stride=1, dil=1, res=False, relu=True, proj=0, seed=0):
    """operands and reference are made once per (regime, shape) and shared by the tests that use them; nobody writes to them"""
    return Case(regime, B, Cin, Cout, H, W, taps, stride, dil, res, relu, proj, seed)


def check(y, ref, what=''):
    """torch.equal, and on failure the count and the first differing (b, c, y, x) with both values"""
    assert tuple(y.shape) == tuple(ref.shape), (what, tuple(y.shape), tuple(ref.shape))
    assert y.dtype == ref.dtype, (what, y.dtype, ref.dtype)
    ref = ref.to(y.device)
    if torch.equal(y, ref):
        return
    bad = y != ref
    n = int(bad.sum())
    i = tuple(int(v) for v in bad.nonzero()[0]) if n else None
    raise AssertionError('%s: %d of %d outputs differ from the exact result; first at (b, c, y, x) = %s: got %r, expected %r' % (
        what or 'convolution', n, y.numel(), i, float(y[i]) if n else None, float(ref[i]) if n else None))


# ---- the cases of tests/test_gpu_conv_exact.py ----------------------------------------------------------------------------------
# spa_conv3x3_bf16: (B, Cin, Cout, H, W, dil, res, relu)
BF16 = [
    (1, 64, 512, 3, 257, 1, False, True),      # 12 tiles of 256 channels: the `rem` = 4 branch of the XCD remap, two channel tiles
    (1, 512, 256, 5, 40, 4, True, True),       # 72 K steps, most dy rows outside the image
    (2, 128, 128, 7, 33, 2, True, False),      # the 128 tile with the residual
    (1, 64, 384, 4, 300, 1, False, True),      # the 128 tile without, three channel tiles
    (1, 64, 192, 1, 255, 3, False, False),     # the 64 tile without the residual, H = 1, dilation 3
    (1, 256, 256, 2, 256, 2, True, True),
    (1, 512, 512, 6, 40, 4, False, True),      # the layer that takes most of the bf16 forward
    (1, 64, 64, 9, 7, 4, True, True),          # W smaller than the halo
]
BF16_REPEATED = (1, 512, 512, 6, 40, 4, False, True)          # k_conv3x3_bf16_stag: six runs, the same bits


def bf16_tiles(B, Cin, Cout, H, W):
    """(channel tile, channel tiles, workgroups) of spa_conv3x3_bf16 (csrc/spa_conv.hip)"""
    bm = 256 if Cout % 256 == 0 else (128 if Cout % 128 == 0 else 64)
    return bm, Cout // bm, B * H * ((W + 255) // 256) * (Cout // bm)


def _light_cases():
    """spa_conv_bf16_light: one case per dispatch branch (Cin, taps, stride, mi) of csrc/spa_convl.hip, the odd sizes, residual
    and ReLU in rotation -> (Cin, Cout, taps, stride, dil, res, relu, B, H, W)"""
    sizes = [(2, 37, 61), (2, 19, 67), (1, 9, 257)]
    branches = []
    for cin, mi, cout in ((32, 4, 64), (64, 4, 192)):
        branches += [(cin, cout, taps, s, mi) for taps in (9, 1) for s in (1, 2)]
    for cin in (128, 256):
        branches += [(cin, 192, 1, s, 4) for s in (1, 2)] + [(cin, 256 if cin == 128 else 128, 1, s, 8) for s in (1, 2)]
    for cin, mi, cout in ((16, 2, 32), (32, 2, 96), (16, 1, 48)):
        branches += [(cin, cout, taps, s, mi) for taps in (9, 1) for s in (1, 2)]
    out = []
    for n, (cin, cout, taps, s, mi) in enumerate(branches):
        B, H, W = sizes[n % 3]
        dil = 2 if (cin, taps, s) == (64, 9, 1) else 1
        out.append((cin, cout, taps, s, dil, n % 2 == 0, n % 4 < 2, B, H, W))
    return out


LIGHT = _light_cases()

# spa_conv3x3_f16s, 3x3 (k_conv3x3_p16 and, with spa_debug_set(ctx, 1, 0), k_conv3x3_f32<SPLIT>): (B, C, H, W, dil, res, relu)
F16S_3X3 = [
    (2, 64, 3, 257, 1, True, True),            # two 256-pixel tiles, one pixel in the second
    (1, 64, 5, 5, 2, False, True),             # narrower than the halo either side
    (1, 64, 6, 257, 4, True, False),           # every row has a dy row outside the image
    (2, 128, 3, 5, 1, False, False),
    (1, 128, 4, 257, 2, True, True),           # three 128-pixel tiles
    (1, 128, 7, 5, 4, False, True),
]
# spa_conv1x1_f16s: (B, Cin, Cout, H, W, res, relu)
F16S_1X1 = [(2, 128, 256, 3, 257, False, False), (1, 256, 512, 7, 5, True, True)]
# spa_conv3x3_s2_f16s with the projection (k_conv3x3_s2_tile and, with spa_debug_set(ctx, 3, 0), k_conv3x3_f32<SPLIT, S = 2>):
# (B, Cin, Cout = width of the opener and of the projection, Hi, Wi)
S2 = [(2, 32, 64, 37, 301), (1, 32, 64, 29, 27), (1, 64, 128, 37, 301), (2, 64, 128, 29, 27)]
# 'wide' only: the forms whose every scale is a power of two and whose float32 output is an exactly representable sum
WIDE_F32_3X3 = (2, 64, 128, 9, 70, 3, True, False)            # spa_conv3x3_f32: (B, Cin, Cout, H, W, dil, res, relu)
WIDE_F32_1X1 = (1, 128, 256, 13, 257)                         # spa_conv1x1_f32: (B, Cin, Cout, H, W)
WIDE_S2_F32 = (2, 32, 64, 37, 301)                            # spa_conv3x3_s2_f32 with the projection
WIDE_SMALL = [(16, 32, 2, 32, False, True, 2, 37, 61), (32, 32, 1, 0, True, True, 2, 19, 67)]   # (Cin, Cout, stride, proj, res, relu, B, H, W)
WIDE_LAYER2 = (2, 37, 61)                                     # spa_drn_layer2_f32 / _f16s: (B, H, W)


def all_cases():
    """every (name, Case) the GPU file uses: test_conv_exact_cpu.py checks each one's bound and condition"""
    for regime in ('unit', 'wide'):
        for B, Cin, Cout, H, W, dil, res, relu in BF16:
            yield 'bf16', case(regime, B, Cin, Cout, H, W, 9, 1, dil, res, relu)
        for Cin, Cout, taps, s, dil, res, relu, B, H, W in LIGHT:
            yield 'light', case(regime, B, Cin, Cout, H, W, taps, s, dil, res, relu)
    for regime in ('planes_x', 'planes_w'):
        for B, C, H, W, dil, res, relu in F16S_3X3:
            yield 'f16s', case(regime, B, C, C, H, W, 9, 1, dil, res, relu)
        for B, Cin, Cout, H, W, res, relu in F16S_1X1:
            yield 'f16s_1x1', case(regime, B, Cin, Cout, H, W, 1, 1, 1, res, relu)
        for B, Cin, Cout, Hi, Wi in S2:
            yield 's2', case(regime, B, Cin, Cout, Hi, Wi, 9, 2, 1, False, True, Cout)
    B, Cin, Cout, H, W, dil, res, relu = WIDE_F32_3X3
    yield 'f32', case('wide', B, Cin, Cout, H, W, 9, 1, dil, res, relu)
    B, Cin, Cout, H, W = WIDE_F32_1X1
    yield 'f32_1x1', case('wide', B, Cin, Cout, H, W, 1, 1, 1, False, False)
    B, Cin, Cout, Hi, Wi = WIDE_S2_F32
    yield 's2_f32', case('wide', B, Cin, Cout, Hi, Wi, 9, 2, 1, False, True, Cout)
    for Cin, Cout, s, proj, res, relu, B, H, W in WIDE_SMALL:
        yield 'small', case('wide', B, Cin, Cout, H, W, 9, s, 1, res, relu, proj)
    B, H, W = WIDE_LAYER2
    yield 'layer2', case('wide', B, 16, 32, H, W, 9, 2, 1, False, True)
