"""Operands on which every SegNet 7x7 entry point has ONE right answer, bit for bit, the float64 references that give it and the
check: the counterpart of tests/conv_exact.py for csrc/spa_segnet*.hip (training forward, dgrad and wgrad, inference encode and
decode; float32, bf16 and split f16 planes).

The tolerance tests (tests/test_gpu_segnet*.py) bound the largest error by a fraction of the largest output and exempt near-tie
pooling windows, at grids of at most 96 workgroups.  Here the operands are small integers times a power of two, so

  * every addend and every partial sum of an output is an integer multiple of one power-of-two unit u,
  * every one of them is below 2^24 u in magnitude (`bound`, asserted when the operands are made),

and a float32 accumulator holds each of them exactly IN ANY ORDER of summation.  The output is the exact sum through the exact
bias, ReLU, pooling (first maximum, equal values frequent), unpooling and power-of-two unscales, and float32 holds it as it is.
`check` is torch.equal: no tolerance, no exempt element.  PREMISE: as in conv_exact.py, a matrix instruction loses no bit of a sum
whose addends and partial sums all fit 24 bits of one unit.  A kernel that differs on these operands is a finding to trace in the
kernel or in this premise; it is never a reason to add a tolerance.

Regimes (each asserts its own bound on the operands or on the reference, never on a kernel's output):
    'wide'      64-channel forms, all families: x in 0..7, w in -3..3, K = 49 * 64 = 3136, 7 * 3 * 3136 + 8 < 2^24; inference bias
                integers in [-8, 8].  Both signs reach the ReLU; equal values inside a 2x2 window are frequent and exact.
    'stats'     training forward: x, w in {-1, 0, 1}.  For every 8 x 32 workgroup tile of the reference, sum |y| and sum y^2 are
                below 2^24 units (asserted per tile and channel): the returned (sum y, sum y^2) float64 pair is the float64 sum
                of the reference bit for bit.
    'planes_x'  split-plane family: x an odd-heavy signed integer up to 4095 (its 12 bits need the low plane), w in {-1, 0, 1}
                (4097 * 1 * 3136 + 16 < 2^24), its low plane zero.  'planes_w' the other way round.
    'tiny'      conv1, all families: pixels k 2^-10, k an integer in -16..16, mean 0, std 1.  alpha s <= 1.47e-8 < 2^-25, so
                `1.f + alpha * s` is 1.0f, powf(1, -0.75) is 1 and the operand is the pixel.  Unit 2^-10 times the weights'.
    'ints'      conv1, bf16 only: pixels integers in -5..5, so LRN is active; x (1 + 2e-5 s)^-0.75 rounds to x in bf16 with the
                nearest rounding boundary >= 1000 float32 ulps away (asserted in float64 when the case is made; 16 178 measured).
    'dec1'      decode1: 'wide' with the pooled map in units of 2^-11 and classifier weights and biases in {-1, 0, 1}, so the logits are
                exact and the two classes are a few units apart.  The softmax is not exact: the probabilities are compared with
                the float64 softmax of the exact logits within the family's PROB_TOL.
    wgrad       dy in -1..1, x in -3..3 (conv1: k 2^-10, k in -3..3): B H W 3 < 2^24, chunk partials are exact in float32 and
                the chunk sum is a float64 sum rounded once.
PREMISE of the conv1 regimes: the float32 training forward with a centre-tap identity weight returns the operand; for 'tiny' it
equals the image bit for bit, for 'ints' its bf16 rounding does.  The GPU file tests that first.

The reference is a float64 sum of 49 per-tap matrix products (as segnet_ref.wgrad_ref), on the CPU or on the device: a float64
64-channel convolution of 2 x 256 x 512 on the CPU is far too slow for a test.  It is cast to float32 with the cast asserted
exact, and cached per (form, regime, shape): the three families share operands.  Nothing here needs a GPU."""
import functools
import zlib

import torch

import conv_exact as ce

F = torch.nn.functional

LIMIT = ce.LIMIT
BIG = ce.BIG
BIAS_MAX = 8
TH, TW = 8, 32                                 # SG_TH, SG_TW: a forward / dgrad / inference workgroup's output tile
WG_TR, WG_TW, WG_MAXCH = 2, 32, 96             # SGW_TR, SGW_TW, SGW_MAXCH: wgrad's tiles and chunk cap
ALPHA = 1e-4 / 5
FAMILIES = ('', '_bf16', '_f16x3')
ZERO3, ONE3 = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)  # conv1's mean and std in every case here
TINY_UNIT = 2.0 ** -10
DEC1_UNIT = 2.0 ** -11

CONV1_SHAPES = [(1, 16, 32), (2, 256, 512), (3, 176, 528)]      # (B, H, W) of the convolution
MAP_SHAPES = [(3, 6, 10), (2, 256, 512), (3, 178, 530)]         # decoders take the (B, H/2, W/2) pooled input
BEYOND_CHIP = [(2, 256, 512), (3, 176, 528), (3, 178, 530)]     # >= 4 workgroups per CU of a 256-CU part
WGRAD_SHAPES = {'conv1': [(1, 16, 32), (2, 256, 512)], 'enc': [(2, 6, 10), (2, 256, 512)], 'dec': [(2, 6, 10), (2, 256, 512)]}

# The only cases that may carry pytest.mark.xfail in tests/test_gpu_segnet_exact.py: (test name, shape).  test_segnet_exact_cpu.py
# asserts that this is a subset of {bf16 conv1 forward, bf16 conv1 encode} x the beyond-chip conv1 shapes.
MARKED = {}


def workgroups(shape):
    B, H, W = shape
    return B * ((H + TH - 1) // TH) * ((W + TW - 1) // TW)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int16)


def _big(g, shape, first_of_each=False):
    """odd-heavy signed integers up to 4095; element 0 (of every image, where a kernel takes one scale per image) is 4095"""
    shape = tuple(shape)
    v = torch.randint(0, BIG + 1, shape, generator=g, dtype=torch.int16)
    v = torch.where(torch.rand(shape, generator=g) < 0.75, v | 1, v)
    v = v * (2 * torch.randint(0, 2, shape, generator=g, dtype=torch.int16) - 1)
    if first_of_each:
        v.view(shape[0], -1)[:, 0] = BIG
    else:
        v.view(-1)[0] = BIG
    return v


# the largest magnitude, in units, an operand of each regime can reach whatever the draw: (x, w); 4097 = |h| + |l| of 4095
REACH = {'tiny': (16, 3), 'ints': (5, 3), 'stats': (1, 1), 'wide': (7, 3), 'dec1': (7, 3), 'planes_x': (BIG + 2, 1),
         'planes_w': (1, BIG + 2)}


def worst_bound(form, regime):
    """the bound of a case from its regime's ranges alone: no draw can exceed it (Conv asserts that of its own operands)"""
    xr, wr = REACH[regime]
    return xr * wr * 49 * (3 if form == 'conv1' else 64) + (2 * BIAS_MAX if regime.startswith('planes') else BIAS_MAX)


def reach(t):
    """the largest |h| + |l| of a split operand, in the operand's own units (conv_exact.Case._assert_bound)"""
    h, l, s = ce.split(t)
    return float((h.abs() + l.abs()).max()) / s


# ---------------------------------------------------------------------------------------------------- layouts, float64 layers
def pack_weight(w):
    """(64,Cin,7,7) -> (49,64,Cp) = (ky * 7 + kx, n, c), Cin 3 zero-padded to 4: the layout every entry point takes"""
    n, cin = w.shape[:2]
    out = torch.zeros((49, n, 4 if cin == 3 else cin), dtype=w.dtype, device=w.device)
    out[:, :, :cin] = w.permute(2, 3, 0, 1).reshape(49, n, cin)
    return out


def forward_taps(w):
    """(64,C,7,7) -> (49,C,64): tap t's matrix of the forward convolution"""
    return w.permute(2, 3, 1, 0).reshape(49, w.shape[1], w.shape[0]).contiguous()


def dgrad_taps(w, rotate=True):
    """(64,C,7,7) -> (49,64,C): the input gradient is the convolution of dy with the weights rotated by 180 degrees and in / out
    exchanged.  rotate False is the mutant without the rotation."""
    if rotate:
        w = w.flip(2, 3)
    return w.permute(2, 3, 0, 1).reshape(49, w.shape[0], w.shape[1]).contiguous()


def conv_taps(x, wk):
    """x (B,H,W,C), wk (49,C,N) -> (B,H,W,N) in x's type: the sum over the 49 taps of (x shifted by the tap) @ wk[tap]"""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 3, 3, 3, 3))
    out = torch.zeros((B, H, W, wk.shape[2]), dtype=x.dtype, device=x.device)
    for b in range(B):
        o = out[b].view(H * W, -1)
        for ky in range(7):
            for kx in range(7):
                o.addmm_(xp[b, ky:ky + H, kx:kx + W].reshape(H * W, C), wk[ky * 7 + kx])
    return out


def wgrad_taps(dy, xin):
    """dW[t][n][c] = sum_p dy[p][n] * xin[p + off(t)][c]: dy (B,H,W,64), xin (B,H,W,C) -> (49,64,C) in dy's type"""
    B, H, W, C = xin.shape
    xp = F.pad(xin, (0, 0, 3, 3, 3, 3))
    g = dy.reshape(-1, 64).t().contiguous()
    out = torch.empty((49, 64, C), dtype=dy.dtype, device=dy.device)
    for ky in range(7):
        for kx in range(7):
            out[ky * 7 + kx] = g @ xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, C)
    return out


def windows(a):
    """(B,H,W,C) -> (B,H/2,W/2,C,4), position r = ky * 2 + kx of each 2x2 window last"""
    B, H, W, C = a.shape
    return a.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def pool_first(a, last=False):
    """-> (the maximum of each 2x2 window, the uint8 index of its FIRST maximum), written out so that no library's tie rule is
    involved.  last True is the mutant that keeps the last maximum."""
    win = windows(a)
    best, arg = win[..., 0], torch.zeros(win.shape[:-1], dtype=torch.uint8, device=a.device)
    for r in range(1, 4):
        v = win[..., r]
        m = (v >= best) if last else (v > best)
        best, arg = torch.where(m, v, best), torch.where(m, torch.full_like(arg, r), arg)
    return best, arg


def unpool(h, idx, transposed=False):
    """h, idx (B,h,w,C) -> (B,2h,2w,C): h at position idx = (gy & 1) * 2 + (gx & 1) of its window, zero elsewhere.  transposed True
    is the mutant that reads the index as (gx & 1) * 2 + (gy & 1)."""
    B, hh, ww, C = h.shape
    out = torch.zeros((B, hh, 2, ww, 2, C), dtype=h.dtype, device=h.device)
    for r in range(4):
        ky, kx = (r & 1, r >> 1) if transposed else (r >> 1, r & 1)
        out[:, :, ky, :, kx, :] = torch.where(idx == r, h, torch.zeros_like(h))
    return out.view(B, 2 * hh, 2 * ww, C)


def gather_pooled(a, idx):
    """a (B,H,W,C), idx (B,H/2,W/2,C) -> a at the position idx selects in each window: the decoder's dgrad at the pooled input"""
    return windows(a).gather(-1, idx.long()[..., None])[..., 0]


def exact32(t, unit=1.0):
    """float64 -> float32, asserted exact and below 2^24 units"""
    assert float(t.abs().max()) < LIMIT * unit
    t32 = t.float()
    assert torch.equal(t32.double(), t)
    return t32


def bf16_margin_ulps(x, v):
    """x the bf16 value the float64 operand v is meant to round to -> the distance of v to the nearer boundary of x's rounding
    interval, in float32 ulps of v (inf where x = v = 0; negative where v rounds elsewhere)"""
    x, v = x.double().abs().reshape(-1), v.double().abs().reshape(-1)
    xb = x.to(torch.bfloat16)
    assert torch.equal(xb.double(), x)
    bits = xb.view(torch.int16).to(torch.int32)
    up = (bits + 1).to(torch.int16).view(torch.bfloat16).double()
    dn = (bits - 1).clamp_min(0).to(torch.int16).view(torch.bfloat16).double()
    ulp = torch.exp2(torch.floor(torch.log2(v.clamp_min(1e-300))) - 23)
    m = torch.minimum(v - (x + dn) / 2, (x + up) / 2 - v) / ulp
    return torch.where(x == 0, torch.full_like(m, float('inf')), m)


def lrn64(img):
    """conv1's operand for mean 0, std 1 in float64: img (B,3,H,W)"""
    img = img.double()
    return img * (1.0 + ALPHA * (img * img).sum(1, keepdim=True)) ** -0.75


# ---------------------------------------------------------------------------------------------------- the cases
class Conv:
    """One 7x7 convolution with exact operands.  form 'conv1' (x the planar (B,3,H,W) image), 'enc' (x a (B,H,W,64) map), 'dec'
    (x the (B,H/2,W/2,64) pooled map with its index map idx) or 'dgrad' (x is dy (B,H,W,64), idx the decoder form's index map;
    the result is the input gradient).  shape = (B, H, W) of the convolution.  x, w (64,Cin,7,7), bias (64), wc (2,64) and bc (2)
    are float32 CPU tensors; xu, wu the powers of two their integers are multiplied by; unit = xu wu."""

    def __init__(self, form, regime, shape):
        assert form in ('conv1', 'enc', 'dec', 'dgrad')
        self.form, self.regime, self.shape = form, regime, tuple(shape)
        B, H, W = shape
        g = _gen(form, regime, shape)
        cin = 3 if form == 'conv1' else 64
        self.K = 49 * cin
        xs = (B, 3, H, W) if form == 'conv1' else (B, H // 2, W // 2, 64) if form == 'dec' else (B, H, W, 64)
        ws = (64, cin, 7, 7)
        self.xu = self.wu = 1.0
        if form == 'conv1':
            assert regime in ('tiny', 'ints', 'stats') and H % 16 == 0 and W % 16 == 0
            if regime == 'tiny':
                x, w, self.xu = _ints(g, xs, -16, 16), _ints(g, ws, -3, 3), TINY_UNIT
            elif regime == 'ints':
                x, w = _ints(g, xs, -5, 5), _ints(g, ws, -3, 3)
            else:
                x, w, self.xu = _ints(g, xs, -1, 1), _ints(g, ws, -1, 1), TINY_UNIT
        else:
            assert regime in ('wide', 'stats', 'planes_x', 'planes_w', 'dec1') and H % 2 == 0 and W % 2 == 0
            assert regime != 'dec1' or form == 'dec'
            if regime in ('wide', 'dec1'):
                x, w = _ints(g, xs, 0, 7), _ints(g, ws, -3, 3)
                self.xu = DEC1_UNIT if regime == 'dec1' else 1.0
            elif regime == 'stats':
                x, w = _ints(g, xs, -1, 1), _ints(g, ws, -1, 1)
            elif regime == 'planes_x':
                x, w = _big(g, xs, first_of_each=True), _ints(g, ws, -1, 1)
            else:
                x, w = _ints(g, xs, -1, 1), _big(g, ws)
                x.view(B, -1)[:, 0] = 1                                  # every image's scale is that of 1 whatever the draw
        self.idx = _ints(g, (B, H // 2, W // 2, 64), 0, 3).to(torch.uint8) if form in ('dec', 'dgrad') else None
        self.unit = self.xu * self.wu
        self.x, self.w = x.float() * self.xu, w.float() * self.wu
        self.bias = _ints(g, (64,), -BIAS_MAX, BIAS_MAX).float() * self.unit
        self.wc = _ints(g, (2, 64), -1, 1).float()
        self.bc = _ints(g, (2,), -1, 1).float()
        self._refs = {}
        self._assert_bound(x, w)

    def _assert_bound(self, xi, wi):
        """every product and partial sum below 2^24 units in ANY order: the sum of the magnitudes of all addends is"""
        if self.regime.startswith('planes'):
            bigt, small = (xi, wi) if self.regime == 'planes_x' else (wi, xi)
            assert not bool(ce.split(small.float())[1].any()), 'the small operand must not carry a low plane'
            assert bool(ce.split(bigt.float())[1].any()), 'the big operand must carry a low plane'
            xm, wm = reach(xi.float()), reach(wi.float())
        else:
            xm, wm = float(xi.abs().max()), float(wi.abs().max())
        self.bound = xm * wm * self.K + (2 * BIAS_MAX if self.regime.startswith('planes') else BIAS_MAX)
        assert self.bound <= worst_bound(self.form, self.regime) < LIMIT, (self.form, self.regime, self.bound)
        if self.regime == 'tiny' or (self.form == 'conv1' and self.regime == 'stats'):
            s = (self.x.double() ** 2).sum(1).max()
            assert ALPHA * float(s) < 2.0 ** -25                          # 1.f + alpha s is 1.f
            one = torch.tensor(1.0) + torch.tensor(ALPHA, dtype=torch.float32) * (self.x * self.x).sum(1)
            assert bool((one == 1.0).all()) and one.dtype == torch.float32
        if self.regime == 'ints':
            self.margin = float(bf16_margin_ulps(self.x, lrn64(self.x)).min())
            assert self.margin >= 1000, self.margin

    # ------------------------------------------------------------------ operands
    def operand64(self, device='cpu', transposed=False):
        """the (B,H,W,C) float64 operand of the convolution at its resolution: conv1's image (its LRN is the identity on these
        operands: the premise), the map, the unpooled map, or dy"""
        x = self.x.to(device).double()
        if self.form == 'conv1':
            return x.permute(0, 2, 3, 1).contiguous()
        if self.form == 'dec':
            return unpool(x, self.idx.to(device), transposed)
        return x

    def wt(self):
        return pack_weight(self.w)

    # ------------------------------------------------------------------ references (cached per device type; nobody writes to them)
    def _cached(self, name, device, make):
        key = (name, torch.device(device).type)
        if key not in self._refs:
            self._refs[key] = make()
        return self._refs[key]

    def y(self, device='cpu'):
        """the exact sums (B,H,W,64) float32: the training forward's output, or dgrad's full-resolution gradient"""
        def make():
            wk = dgrad_taps(self.w) if self.form == 'dgrad' else forward_taps(self.w)
            y = exact32(conv_taps(self.operand64(device), wk.to(device).double()), self.unit)
            if self.regime == 'stats':
                self._assert_tiles(y)
            return y
        return self._cached('y', device, make)

    def _assert_tiles(self, y):
        """'stats': per workgroup tile and channel, sum |y| and sum y^2 below 2^24 units, so the float32 partial sums are exact"""
        B, H, W, C = y.shape
        yp = F.pad(y.double() / self.unit, (0, 0, 0, -W % TW, 0, -H % TH))
        t = yp.view(B, yp.shape[1] // TH, TH, yp.shape[2] // TW, TW, C)
        assert float(t.abs().sum((2, 4)).max()) < LIMIT and float((t * t).sum((2, 4)).max()) < LIMIT

    def stats(self, device='cpu'):
        """(sum y, sum y^2) (2,64) float64: exact in float64, every term an integer multiple of unit^2 far below 2^53"""
        def make():
            y = self.y(device).double()
            return torch.stack([y.sum((0, 1, 2)), (y * y).sum((0, 1, 2))])
        return self._cached('stats', device, make)

    def pooled_grad(self, device='cpu'):
        """the decoder form of dgrad: the gradient at the pooled input"""
        return self._cached('pg', device, lambda: gather_pooled(self.y(device), self.idx.to(device)).contiguous())

    def biased(self, device='cpu'):
        def make():
            v = self.y(device).double() + self.bias.to(device).double()
            if self.form != 'dec':
                assert bool((v < 0).any()) and bool((v > 0).any())        # both signs reach the ReLU
            return exact32(v, self.unit)
        return self._cached('biased', device, make)

    def encoded(self, device='cpu'):
        """inference encode: (maxpool2x2(relu(y + bias)), first-maximum index), each (B,H/2,W/2,64)"""
        return self._cached('enc', device, lambda: pool_first(torch.relu(self.biased(device))))

    def logits64(self, device='cpu'):
        """decode1: the classifier on y + bias, exact integers of unit in float64, (B,2,H,W)"""
        def make():
            z = self.biased(device).double() @ self.wc.to(device).double().t() + self.bc.to(device).double()
            assert float(z.abs().max()) < LIMIT * self.unit
            return z.permute(0, 3, 1, 2).contiguous()
        return self._cached('z', device, make)

    def tie_fraction(self, device='cpu'):
        """share of the 2x2 windows of relu(y + bias) whose maximum occurs more than once"""
        win = windows(torch.relu(self.biased(device)))
        return float(((win == win.max(-1, keepdim=True).values).sum(-1) > 1).double().mean())


class Wgrad:
    """One weight gradient with exact operands: dy (B,H,W,64) in -1..1; the input form x (, idx) in -3..3 (conv1: k 2^-10)."""

    def __init__(self, form, shape):
        assert form in ('conv1', 'enc', 'dec')
        self.form, self.shape = form, tuple(shape)
        B, H, W = shape
        g = _gen('wgrad', form, shape)
        xs = (B, 3, H, W) if form == 'conv1' else (B, H // 2, W // 2, 64) if form == 'dec' else (B, H, W, 64)
        self.unit = TINY_UNIT if form == 'conv1' else 1.0
        self.x = _ints(g, xs, -3, 3).float() * self.unit
        self.dy = _ints(g, (B, H, W, 64), -1, 1).float()
        self.idx = _ints(g, xs, 0, 3).to(torch.uint8) if form == 'dec' else None
        self.bound = B * H * W * 3
        assert self.bound < LIMIT and float(self.x.abs().max()) <= 3 * self.unit and float(self.dy.abs().max()) <= 1
        if form == 'conv1':
            assert ALPHA * 27 * self.unit ** 2 < 2.0 ** -25
        self._refs = {}

    def chunks(self):
        """(number of 2 x 32 tiles, number of chunks): sg_wgrad_plan"""
        B, H, W = self.shape
        tiles = B * (H // WG_TR) * ((W + WG_TW - 1) // WG_TW)
        return tiles, min(tiles, WG_MAXCH)

    def operand64(self, device='cpu'):
        x = self.x.to(device).double()
        if self.form == 'conv1':
            return F.pad(x.permute(0, 2, 3, 1), (0, 1)).contiguous()          # channel 3 is zero
        return unpool(x, self.idx.to(device)) if self.form == 'dec' else x

    def dw(self, device='cpu'):
        key = torch.device(device).type
        if key not in self._refs:
            self._refs[key] = exact32(wgrad_taps(self.dy.to(device).double(), self.operand64(device)), self.unit)
        return self._refs[key]


@functools.lru_cache(maxsize=None)
def conv(form, regime, shape):
    """operands and references are made once per (form, regime, shape) and shared by the families; nobody writes to them"""
    return Conv(form, regime, shape)


@functools.lru_cache(maxsize=None)
def wgrad(form, shape):
    return Wgrad(form, shape)


def check(y, ref, what=''):
    """torch.equal, and on failure the count and the first differing index with both values"""
    assert tuple(y.shape) == tuple(ref.shape), (what, tuple(y.shape), tuple(ref.shape))
    assert y.dtype == ref.dtype, (what, y.dtype, ref.dtype)
    ref = ref.to(y.device)
    if torch.equal(y, ref):
        return
    bad = y != ref
    n = int(bad.sum())
    i = tuple(int(v) for v in bad.nonzero()[0]) if n else None
    raise AssertionError('%s: %d of %d outputs differ from the exact result; first at %s: got %r, expected %r' % (
        what or 'output', n, y.numel(), i, float(y[i]) if n else None, float(ref[i]) if n else None))


# ---------------------------------------------------------------------------------------------------- the GPU file's cases
def forward_regimes(form, family):
    if form == 'conv1':
        return ['tiny', 'stats'] + (['ints'] if family == '_bf16' else [])
    return ['wide', 'stats'] + (['planes_x', 'planes_w'] if family == '_f16x3' else [])


def infer_regimes(form, family):
    """encode ('conv1', 'enc'), decode ('dec') and dgrad"""
    if form == 'conv1':
        return ['tiny'] + (['ints'] if family == '_bf16' else [])
    return ['wide'] + (['planes_x', 'planes_w'] if family == '_f16x3' else [])


def shapes(form):
    return CONV1_SHAPES if form == 'conv1' else MAP_SHAPES


def forward_cases():
    """(family, form, regime, shape) of segnet_train_forward*"""
    return [(fam, form, r, s) for fam in FAMILIES for form in ('conv1', 'enc', 'dec') for r in forward_regimes(form, fam)
            for s in shapes(form)]


def dgrad_cases():
    return [(fam, r, s) for fam in FAMILIES for r in infer_regimes('dgrad', fam) for s in MAP_SHAPES]


def wgrad_cases():
    return [(fam, form, s) for fam in FAMILIES for form in ('conv1', 'enc', 'dec') for s in WGRAD_SHAPES[form]]


def encode_cases():
    return [(fam, form, r, s) for fam in FAMILIES for form in ('conv1', 'enc') for r in infer_regimes(form, fam)
            for s in shapes(form)]


def decode_cases():
    return [(fam, r, s) for fam in FAMILIES for r in infer_regimes('dec', fam) for s in MAP_SHAPES]


def decode1_cases():
    return [(fam, s) for fam in FAMILIES for s in CONV1_SHAPES]


def conv_keys():
    """every (form, regime, shape) of a Conv the GPU file uses"""
    keys = {(form, r, s) for fam, form, r, s in forward_cases() + encode_cases()}
    keys |= {('dgrad', r, s) for fam, r, s in dgrad_cases()} | {('dec', r, s) for fam, r, s in decode_cases()}
    keys |= {('dec', 'dec1', s) for fam, s in decode1_cases()}
    return sorted(keys)


def marks(test, shape):
    """the pytest marks of one GPU case: MARKED's, nothing else"""
    import pytest
    reason = MARKED.get((test, tuple(shape)))
    return [pytest.mark.xfail(reason=reason, strict=False)] if reason else []
