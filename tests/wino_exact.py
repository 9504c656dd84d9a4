"""Operands on which the Winograd convolutions (csrc/spa_wino.hip: spa_conv3x3_wino_f32, spa_conv3x3_wino4_f32,
spa_conv3x3_wino4_f16s) have ONE right answer, bit for bit, the premises that make it so, the reference and the check.

Every other test of this path bounds the error by 1e-5 of the largest output; at K = 9 x 256 .. 512 one dropped, doubled or
misplaced (channel, position) term, or a wrong low plane (2^-11 of an operand), is inside that bound.  tests/conv_exact.py
left the Winograd forms out because G has thirds and fifteenths.  But they live ONLY in G, which the host applies in float64
(Engine.winograd_weights); in the kernels wino4_bt has integer coefficients, wino4_at powers of two (1/8 .. 8), and every scale
(2^(14 - e - p_i - p_j) of V, t_ij of U, cs, 2^(e - 14)) is a power of two.  15 G is dyadic,

    15 G = (7.5, 0, 0), (2.5, 2.5, 2.5), (2.5, -2.5, 2.5), (16, 8, 4), (.5, -1, 2), (0, 0, 7.5),

so for weights w = 225 k with integer k, U = G w G^T = (30 G) k (30 G)^T / 4 is an exact multiple of 1/4 with few significant
bits; V = B^T x B is an integer for integer x; every later step is a sum of dyadic numbers.  If every partial sum fits 24 bits
of its addends' smallest unit, float32 holds it exactly in any order, with or without fused multiply-adds, and the layer's
output is 225 conv(x, k) + bias + residual through the ReLU, exactly.  F(2x2,3x3) has G of halves only: w = k there.

PREMISES, asserted on the data of every case when it is made (`Case._premises`; the figures are kept in `Case.bounds`):
  (a) Engine.winograd_weights(w, tile).double() IS U computed in integer arithmetic.  (With G as float64 fractions it was not:
      taps that cancel exactly left 1e-15 where U is zero.  engine.py now multiplies by 30 G and divides once by 900.);
  (b) winograd_weights_split: h + l = t U exactly with t = 2^(p_i + p_j) / cs a power of two, the small operand's low plane zero;
  (c) the big operand of a plane regime carries a low plane: at least `LOW_SHARE` of its elements, and at least one element in
      every position (where U is non-zero at all) — no position is exempt in any case below;
  (d) V computed in float32 in wino4_bt's expression order is the integer result, and its planes at the scale 2^(14 - e - psum),
      e from the amax word as wino_amax_exp reads it, are exact (h + l = s V);
  (e) per position, the largest sum over the channels of |plane of V| |plane of U|, in units of the product of the two planes'
      lowest set bits, is below 2^24 — for h.h, h.l and l.h each, for the three in ONE accumulator (the GEMM kernels keep one)
      in the smallest of the three units, and for the float32 GEMM on the unsplit V and U;
  (f) the output transform: wino4_at applied twice in float32 to the exact M (x cs x 2^(e - 14), a power of two) equals its
      float64 evaluation, and the sum of the magnitudes of ALL 36 addends A_ia A_jb M_ab of an output, plus |bias|, |residual|,
      is below 2^24 of the smallest unit among them.  (Every first-stage value is used by an output with coefficient 1 — row 0
      of A^T is ones over positions 0..4, position 5 enters row 3 only, with 1 — so the first stage's partial sums are bounded
      by the same figure, in a unit no smaller.)
The premise of conv_exact.py about the matrix instructions is used here in a wider form: the addends of ONE accumulator have
different units (l.h, h.l, h.h), and the sum stays exact when it fits 24 bits of the smallest one.

Regimes (|bias|, |residual| <= 8; the largest |x| is planted at element 0, so the amax word is known whatever the draw).  The
GEMM alone would leave room for more (22.7 bits at 512 -> 512 in 'wide'); what binds is (f): F(4x4,3x3) amplifies — position
(0, 0) alone contributes |V_00| |U_00| <= 196 max|x| x 56.25 |k| — and the addends of an output are multiples of 1/4.
    'wide'      x in -3..3, k in {-1, 0, 1} dense: no low plane anywhere; runs at every channel count up to 512 -> 512
                (GEMM 22.7 bits, output transform 23.4 there).
    'planes_w'  k in -31..31, x in {-1, 0, 1} with 4 non-zero channels per pixel on average: 12 % of U has a non-zero low plane,
                V has none.  A position whose row of 30 G is (32, 16, 8) or (1, -2, 4) needs |k| up to 63 for 12 significant bits:
                output channel z carries, at input channel 0, a kernel of magnitudes 32..63 made for position z (`_plant_u`).
    'planes_x'  x in -120..120 dense, ONE tap of +-1 per output channel, the input channels going round: 6-13 % of V has a
                non-zero low plane, U has none.  A low plane at positions (3, 3), (3, 4), (4, 4) needs |V| >= 2048 from 36 |x|, and
                that one addend, times 64 from A^T, is 2^21 units of (f): a second tap per output channel does not fit.  Each
                position gets a patch made for it (`_plant_v`), no larger than its low plane needs.  The sums over the channels
                are the other regimes' business; here every element of V is an addend of some output, so a wrong plane shows.
                On the 2 x 9 x 7 map at dilation 4 a sub-grid has 3 x 2 pixels and (c) cannot hold from position 19 on (|V| stays
                below 2048): that map runs 'planes_x' at dilations 1 and 2 only, and no case lowers the share or exempts a position.
The kernels drop l.l by design, so only one operand may carry a low plane.

The reference is torch's float64 convolution on the CPU of (x, w), bias, residual, ReLU, cast to float32 with the cast asserted
exact; for the one large shape 9 per-tap float64 matrix products (`taps64`, held to F.conv2d at a small shape).  `check` is
conv_exact.check: torch.equal, no tolerance, no exempt element.  Nothing here needs a GPU."""
import functools
import importlib
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact as ce  # noqa: E402

F = torch.nn.functional
check = ce.check
LIMIT, BR_MAX = ce.LIMIT, ce.BR_MAX
REGIMES = ('wide', 'planes_w', 'planes_x')
LOW_SHARE = 0.05
PLANT_K = 63                                             # the planted kernels of 'planes_w' (premise (c))
W_BULK, W_PIXELS = 31, 4.0                               # 'planes_w': |k| of the bulk, non-zero channels per pixel
X_MAX, X_TAPS = 120, 1                                   # 'planes_x': |x|, taps of +-1 per output channel
P4 = (4, 4, 4, 3, 3, 4)                                  # wino4_psum's table 0x433444, lowest nibble first

G30 = [[15, 0, 0], [5, 5, 5], [5, -5, 5], [32, 16, 8], [1, -2, 4], [0, 0, 15]]          # 30 G of F(4x4,3x3)
G2 = [[2, 0, 0], [1, 1, 1], [1, -1, 1], [0, 0, 2]]                                      # 2 G of F(2x2,3x3)
BT4 = [[2, -3, -4, 3, 2, 0], [0, -2, 1, 5, 2, 0], [0, -2, 5, -1, -2, 0], [0, 2, 1, -2, -1, 0], [0, 1, -2, -1, 2, 0], [0, 2, -3, -4, 3, 2]]
AT4 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, .5, -2, 0], [0, 1, 1, .25, 4, 0], [0, 1, -1, .125, -8, 1]]
BT2 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
AT2 = [[1, 1, 1, 0], [0, 1, -1, -1]]


def engine():
    return importlib.import_module('superpixel-align_amd.engine').Engine


# ---- the device code restated (csrc/spa_wino_dev.h, spa_wino.hip) -----------------------------------------------------------------
def psum(z, p=P4):
    return p[z // 6] + p[z % 6]


def amax_exp(word):
    """wino_amax_exp of the bit pattern of a float32"""
    e = (int(word) >> 23) - 127
    e = max(-100, min(100, e))
    return 0 if int(word) == 0 else e


def amax_word(v):
    return int(np.float32(v).view(np.uint32))


def bt4(x):
    """wino4_bt, the header's expression order"""
    return [2.0 * (x[0] + x[4]) + 3.0 * (x[3] - x[1]) - 4.0 * x[2],
            2.0 * (x[4] - x[1]) + x[2] + 5.0 * x[3],
            5.0 * x[2] - 2.0 * (x[1] + x[4]) - x[3],
            2.0 * (x[1] - x[3]) + x[2] - x[4],
            (x[1] - x[3]) + 2.0 * (x[4] - x[2]),
            2.0 * (x[1] + x[5]) + 3.0 * (x[4] - x[2]) - 4.0 * x[3]]


def at4(x, eighth=0.125):
    """wino4_at"""
    return [((x[0] + x[1]) + x[2]) + (x[3] + x[4]),
            (x[1] - x[2]) + (0.5 * x[3] - 2.0 * x[4]),
            (x[1] + x[2]) + (0.25 * x[3] + 4.0 * x[4]),
            ((x[1] - x[2]) + (eighth * x[3] - 8.0 * x[4])) + x[5]]


def bt2(x):
    """k_wino_in"""
    return [x[0] - x[2], x[1] + x[2], x[2] - x[1], x[1] - x[3]]


def at2(x):
    """k_wino_out"""
    return [(x[0] + x[1]) + x[2], (x[1] - x[2]) - x[3]]


def along(fn, t, axis):
    return torch.stack(fn(list(t.unbind(axis))), axis)


def transform_in(p, tile):
    """(T, n, n, C) patches -> V (T, n, n, C) in the kernels' order: k_wino4_in transforms each row's columns first, k_wino_in the
    rows first; the type is the argument's"""
    return along(bt4, along(bt4, p, 2), 1) if tile == 4 else along(bt2, along(bt2, p, 1), 2)


def transform_out(m, tile, eighth=0.125):
    """(T, n, n, K) -> (T, tile, tile, K): both out kernels go down the columns first (A^T m), then along the rows"""
    at = (lambda v: at4(v, eighth)) if tile == 4 else at2
    return along(at, along(at, m, 1), 2)


class Geom:
    """the tiling of the sub-grids of a dilation (wino4_geom / wino_geom) and the tile decode (wino_tile) for all tiles at once"""

    def __init__(self, B, H, W, d, tile, interleaved=None, swap_sub=False):
        self.B, self.H, self.W, self.d, self.tile = B, H, W, d, tile
        hs, ws = (H + d - 1) // d, (W + d - 1) // d
        self.th, self.tw = (hs + tile - 1) // tile, (ws + tile - 1) // tile
        self.T = B * d * d * self.th * self.tw
        self.Tpad = (self.T + 255) // 256 * 256
        t = torch.arange(self.T)
        if (d > 2) if interleaved is None else interleaved:
            rw = self.tw * d
            gx, t = t % rw, t // rw
            sx, tx = gx % d, gx // d
            ty, t = t % self.th, t // self.th
            sy, b = t % d, t // d
        else:
            tx, t = t % self.tw, t // self.tw
            ty, t = t % self.th, t // self.th
            sx, t = t % d, t // d
            sy, b = t % d, t // d
        if swap_sub:
            sx, sy = sy, sx
        self.b, self.sy, self.sx, self.ty, self.tx = b, sy, sx, ty, tx

    def patch_coords(self):
        """(y, x) of the (tile + 2)^2 input pixels of every tile: (T, n) each"""
        a = torch.arange(self.tile + 2)
        return (self.sy[:, None] + (self.tile * self.ty[:, None] - 1 + a) * self.d,
                self.sx[:, None] + (self.tile * self.tx[:, None] - 1 + a) * self.d)

    def out_coords(self):
        a = torch.arange(self.tile)
        return (self.sy[:, None] + (self.tile * self.ty[:, None] + a) * self.d,
                self.sx[:, None] + (self.tile * self.tx[:, None] + a) * self.d)

    def gather(self, x, wrap=False):
        """x (B, C, H, W) -> patches (T, n, n, C), zero outside the image.  wrap: the column is not bounded, a pixel left or right of
        the image is read from the flat address, i.e. from the neighbouring row"""
        B, C, H, W = x.shape
        flat = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
        ys, xs = self.patch_coords()
        ys, xs = ys[:, :, None], xs[:, None, :]
        ok = (ys >= 0) & (ys < H) & ((xs >= 0) & (xs < W) if not wrap else torch.ones_like(xs, dtype=torch.bool))
        addr = (self.b[:, None, None] * H + ys) * W + xs
        ok = ok & (addr >= 0) & (addr < B * H * W)
        p = flat[addr.clamp(0, B * H * W - 1)]
        return p * ok[..., None].to(p.dtype)

    def scatter(self, o, clip_rows=0, strict=True):
        """o (T, tile, tile, K) -> y (B, K, H, W); what no tile writes stays NaN.  clip_rows: rows the clipping loses; strict: every
        pixel is written exactly once"""
        K = o.shape[-1]
        y = torch.full((self.B * self.H * self.W, K), float('nan'), dtype=o.dtype)
        ys, xs = self.out_coords()
        ys, xs = ys[:, :, None], xs[:, None, :]
        ok = (ys < self.H - clip_rows) & (xs < self.W)
        addr = ((self.b[:, None, None] * self.H + ys) * self.W + xs)[ok]
        assert not strict or addr.unique().numel() == addr.numel() == self.B * (self.H - clip_rows) * self.W
        y[addr] = o[ok]
        return y.view(self.B, self.H, self.W, K).permute(0, 3, 1, 2).contiguous()


def lsb(t):
    """the smallest lowest set bit among the non-zero elements of a float64 tensor, inf when there is none"""
    v = t.detach().numpy().reshape(-1)
    v = v[v != 0]
    if v.size == 0:
        return math.inf
    m, e = np.frexp(np.abs(v))
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    return float(np.min(low * np.exp2(e.astype(np.float64) - 53)))


def significant_bits(v):
    """of an integer: from its leading bit to its lowest set bit"""
    v = abs(int(v))
    return 0 if v == 0 else v.bit_length() - ((v & -v).bit_length() - 1)


def planes(v, s):
    """h = rn16(s v), l = rn16(s v - h) of a float64 tensor holding exact values, s a power of two: (h, l) float64, exactness asserted"""
    vs = (v * s).float()
    assert torch.equal(vs.double(), v * s)
    h = vs.half().float()
    l = (vs - h).half().float()
    assert torch.equal(h.double() + l.double(), v * s), 'two half-precision planes do not hold the value'
    return h.double(), l.double()


def u_exact(k, tile):
    """U = G w G^T in integer arithmetic: (n n, Cout, Cin) float64, w = 225 k (tile 4) or k (tile 2)"""
    Gi = torch.tensor(G30 if tile == 4 else G2, dtype=torch.int64)
    u = torch.einsum('ij,kcjl,ml->imkc', Gi, k.to(torch.int64), Gi)
    assert int(u.abs().max()) < 2 ** 40
    n = Gi.shape[0]
    return u.reshape(n * n, k.shape[0], k.shape[1]).double() / 4


def taps64(x, w, dil, device='cpu'):
    """conv3x3(x, w; padding = dilation) as 9 per-tap float64 matrix products: (B, Cout, H, W) float64 on `device`"""
    B, C, H, W = x.shape
    xp = F.pad(x.to(device).double(), (dil, dil, dil, dil)).permute(0, 2, 3, 1).contiguous()
    wd = w.to(device).double()
    y = torch.zeros((B, H, W, w.shape[0]), dtype=torch.float64, device=device)
    for ky in range(3):
        for kx in range(3):
            y += xp[:, ky * dil:ky * dil + H, kx * dil:kx * dil + W, :] @ wd[:, :, ky, kx].t()
    return y.permute(0, 3, 1, 2)


class Case:
    """One Winograd layer with exact operands: x (B,Cin,H,W), k and w = 225 k or k (Cout,Cin,3,3), bias (Cout), res (B,Cout,H,W) or
    None, float64 CPU tensors holding integers; amax_word the word handed to the split form (twice the true maximum with amax2)"""

    def __init__(self, regime, B, Cin, Cout, H, W, dil=1, res=False, relu=True, tile=4, amax2=False, seed=0):
        assert regime in REGIMES and tile in (2, 4) and (tile == 4 or regime == 'wide')
        self.regime, self.dil, self.relu, self.tile, self.amax2 = regime, dil, relu, tile, amax2
        self.shape = (B, Cin, Cout, H, W)
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * Cin + 31 * Cout + 17 * H + W + 5 * dil + len(regime))

        def ints(shape, lo, hi):
            return torch.randint(lo, hi + 1, shape, generator=g).double()

        def keep(shape, density):
            return (torch.rand(shape, generator=g) < density).double()
        xs, ws = (B, Cin, H, W), (Cout, Cin, 3, 3)
        self.geom = Geom(B, H, W, dil, tile)
        if regime == 'wide':
            xmax, x, k = 3, ints(xs, -3, 3), ints(ws, -1, 1)
        elif regime == 'planes_w':
            kb = W_BULK
            xmax, x = 1, (2 * ints(xs, 0, 1) - 1) * keep(xs, min(1.0, W_PIXELS / Cin))
            k = ints(ws, -kb, kb)
            self._plant_u(k, g)
        else:
            xmax = X_MAX
            x = ints(xs, -xmax, xmax)
            # X_TAPS taps of +-1 per output channel, their input channels going round so that every channel is used
            k = torch.zeros(ws, dtype=torch.float64)
            nt = X_TAPS
            co = torch.arange(Cout).repeat_interleave(nt)
            k[co, torch.arange(Cout * nt) % Cin, torch.randint(0, 3, (Cout * nt,), generator=g), torch.randint(0, 3, (Cout * nt,), generator=g)] = \
                2 * ints((Cout * nt,), 0, 1) - 1
            self._plant_v(x, xmax, g)
        x.view(-1)[0] = xmax                                   # the tracked maximum, whatever the draw
        self.x, self.k, self.w = x, k, k * (225 if tile == 4 else 1)
        self.bias = ints((Cout,), -BR_MAX, BR_MAX)
        self.res = ints((B, Cout, H, W), -BR_MAX, BR_MAX) if res else None
        self.amax_word = amax_word(xmax * (2 if amax2 else 1))
        self._refs = {}
        self.bounds = {}
        self._premises()

    def _plant_u(self, k, g):
        """premise (c) at EVERY position: output channel z gets, at input channel 0, a kernel whose U at position z has more than
        11 significant bits — every tap with the sign of its coefficient in (30 G)_i x (30 G)_j and a magnitude in 32..63"""
        Gi = torch.tensor(G30, dtype=torch.float64)
        for z in range(36):
            coef = torch.outer(Gi[z // 6], Gi[z % 6])
            for attempt in range(1000):
                kern = torch.sign(coef) * torch.randint(32, PLANT_K + 1, (3, 3), generator=g).double()
                if significant_bits(int((coef * kern).sum())) > 11:
                    break
            else:
                raise AssertionError('(c) cannot hold at position %d' % z)
            k[z, 0] = kern

    def _plant_v(self, x, xmax, g):
        """the same for V: position z gets, in channel z mod Cin of the tile with the most pixels inside the image (of image 0, or
        of the last image once the channels are used up), pixels with the sign of their coefficient in B^T_i x B^T_j and a
        magnitude in xmax / 2 .. xmax"""
        geom, Cin = self.geom, x.shape[1]
        ys, xs = geom.patch_coords()
        real = ((ys >= 0) & (ys < geom.H))[:, :, None] & ((xs >= 0) & (xs < geom.W))[:, None, :]
        count = real.sum(dim=(1, 2))
        first = int((count * (geom.b == 0)).argmax())
        last = int((count * (geom.b == geom.B - 1)).argmax())
        assert 36 <= 2 * Cin and geom.B >= 2
        Bt = torch.tensor(BT4, dtype=torch.float64)
        for z in range(36):
            t = first if z < Cin else last
            coef = torch.outer(Bt[z // 6], Bt[z % 6]) * real[t]
            if float(coef.abs().sum()) * xmax < 2048:
                raise AssertionError('(c) cannot hold at position %d: the map is too small' % z)
            lo = int(math.ceil(2048.0 / float(coef.abs().sum())))          # no larger than the low plane needs: the bound (f) feels it
            for attempt in range(1000):
                patch = torch.sign(coef) * torch.randint(lo, min(lo + 8, xmax) + 1, (6, 6), generator=g).double()
                if significant_bits(int((coef * patch).sum())) > 11:
                    break
            else:
                raise AssertionError('(c) cannot hold at position %d' % z)
            on = coef != 0
            x[int(geom.b[t]), z % Cin, ys[t][:, None].expand(6, 6)[on], xs[t][None, :].expand(6, 6)[on]] = patch[on]

    # ------------------------------------------------------------------ the exact Winograd domain
    def v64(self):
        g, n = self.geom, self.tile + 2
        Bt = torch.tensor(BT4 if self.tile == 4 else BT2, dtype=torch.float64)
        return torch.einsum('ia,tabc,jb->tijc', Bt, g.gather(self.x), Bt)                     # (T, n, n, Cin)

    def _premises(self):
        Engine = engine()
        tile, n = self.tile, self.tile + 2
        B, Cin, Cout, H, W = self.shape
        T = self.geom.T
        # (a) the host's U is the exact one
        U = u_exact(self.k, tile)
        self.u = Engine.winograd_weights(self.w, tile)                    # what the kernels are handed: (n n, Cout, Cin) float32
        assert torch.equal(self.u.double(), U), '(a) winograd_weights is not the exact U'
        # (d) V in float32 in the kernel's order is the integer result
        V = self.v64()
        assert torch.equal(V, V.round()) and float(V.abs().max()) < LIMIT
        v32 = transform_in(self.geom.gather(self.x.float()), tile)
        assert v32.dtype == torch.float32 and torch.equal(v32.double(), V), '(d) the float32 input transform is not exact'
        Vz = V.reshape(T, n * n, Cin).permute(1, 0, 2).contiguous()                               # (z, T, Cin)
        bits = {}

        def reach(a, b):
            """log2 of the largest sum over the channels of |a| |b|^T in units of the two operands' lowest set bits"""
            ua, ub = lsb(a), lsb(b)
            if math.isinf(ua) or math.isinf(ub):
                return -math.inf, math.inf
            return float((a.abs() @ b.abs().t()).max()), ua * ub

        def note(name, s, unit):
            if s > 0:
                bits[name] = max(bits.get(name, -math.inf), math.log2(s / unit))

        for z in range(n * n):
            note('f32', *reach(Vz[z], U[z]))
        M = torch.einsum('ztc,zkc->ztk', Vz, U)                                                  # exact: far below 2^53
        if tile == 4:
            # (b) the split weights
            u2, cs = self.u2, self.cs = Engine.winograd_weights_split(self.w)
            cs64 = torch.from_numpy(cs).double()
            mant, _ = torch.frexp(cs64)
            assert bool((mant == 0.5).all()), '(b) cs is not a power of two'
            t = torch.tensor([2.0 ** psum(z) for z in range(36)], dtype=torch.float64) / cs64
            Uh = u2[:, :, :, 0, :].reshape(36, Cout, Cin).double()
            Ul = u2[:, :, :, 1, :].reshape(36, Cout, Cin).double()
            assert torch.equal(Uh + Ul, U * t.view(36, 1, 1)), '(b) h + l is not t U'
            e = amax_exp(self.amax_word)
            assert 2.0 ** (e + 1) > float(self.x.abs().max()), 'amax >= max |x|'
            inv = 2.0 ** (e - 14)
            Vh, Vl = torch.empty_like(Vz), torch.empty_like(Vz)
            for z in range(36):
                s = 2.0 ** (14 - e - psum(z))
                Vh[z], Vl[z] = planes(Vz[z], s)                                                   # (d) exact planes
                assert float(Vh[z].abs().max()) < 2.0 ** 15
                assert s * float(t[z]) * float(cs64[z]) * inv == 1.0
            # (b), (c) who carries a low plane
            if self.regime != 'planes_w':
                assert not bool(Ul.any()), '(b) the small operand (U) carries a low plane'
            if self.regime != 'planes_x':
                assert not bool(Vl.any()), '(b) the small operand (V) carries a low plane'
            if self.regime != 'wide':
                low, whole = (Ul, U) if self.regime == 'planes_w' else (Vl, Vz)
                share = float((low != 0).double().mean())
                self.bounds['low share'] = share
                assert share >= LOW_SHARE, ('(c)', share)
                for z in range(36):
                    assert bool(low[z].any()) or not bool(U[z].any()), '(c) no low plane at position %d' % z
            # (e) the three accumulations, and all three in one accumulator
            for z in range(36):
                hh, hl, lh = reach(Vh[z], Uh[z]), reach(Vh[z], Ul[z]), reach(Vl[z], Uh[z])
                for name, (s, unit) in (('h.h', hh), ('h.l', hl), ('l.h', lh)):
                    note(name, s, unit)
                total = float(((Vh[z].abs() @ Uh[z].abs().t()) + (Vh[z].abs() @ Ul[z].abs().t()) + (Vl[z].abs() @ Uh[z].abs().t())).max())
                note('one accumulator', total, min(hh[1], hl[1], lh[1]))
        # (f) the output transform on the exact M
        m = M.permute(1, 0, 2).reshape(T, n, n, Cout)
        m32 = m.float()
        assert torch.equal(m32.double(), m), '(f) M does not fit float32'
        o32, o64 = transform_out(m32, tile), transform_out(m, tile)
        assert o32.dtype == torch.float32 and torch.equal(o32.double(), o64), '(f) the float32 output transform is not exact'
        At = torch.tensor(AT4 if tile == 4 else AT2, dtype=torch.float64)
        amin = [float(At[:, a][At[:, a] != 0].abs().min()) for a in range(n)]
        unit = min([1.0] + [lsb(m[:, a, b]) * amin[a] * amin[b] for a in range(n) for b in range(n)])
        reach_o = float(torch.einsum('jb,tibk->tijk', At.abs(), torch.einsum('ia,tabk->tibk', At.abs(), m.abs())).max())
        reach_o += BR_MAX + (BR_MAX if self.res is not None else 0)
        note('output transform', reach_o, unit)
        self.bounds.update(bits)
        for name, b in bits.items():
            assert b < 24, (name, b, self.regime, self.shape)
        self._o64 = o64                                     # the exact tiles, for ref64's cross-check at the small shapes

    # ------------------------------------------------------------------ the reference
    def pre64(self, device='cpu', taps=False):
        """conv + bias + residual in front of the ReLU, float64: F.conv2d on the CPU, or (taps, or any other device) `taps64`"""
        if device == 'cpu' and not taps:
            y = F.conv2d(self.x, self.w, None, 1, self.dil, self.dil)
        else:
            y = taps64(self.x, self.w, self.dil, device)
        y = y + self.bias.to(y.device).view(1, -1, 1, 1)
        return y if self.res is None else y + self.res.to(y.device)

    def ref(self, device='cpu', taps=False):
        """the exact output as float32 (the cast asserted exact), on `device`"""
        key = (str(device), taps)
        if key not in self._refs:
            pre = self.pre64(device, taps)
            assert bool((pre < 0).any()) and bool((pre > 0).any()), 'both signs in front of the ReLU'
            y = torch.relu(pre) if self.relu else pre
            assert float(y.abs().max()) < LIMIT and torch.equal(y, y.round())
            y32 = y.float()
            assert torch.equal(y32.double(), y)
            self._refs[key] = y32
        return self._refs[key]

    def scatter_exact(self):
        """the exact tiles of premise (f) as an image: conv(x, w) by the Winograd route in float64, for the self-check"""
        return self.geom.scatter(self._o64)


@functools.lru_cache(maxsize=None)
def case(regime, B, Cin, Cout, H, W, dil=1, res=False, relu=True, tile=4, amax2=False, seed=0):
    """operands, premises and reference are made once per key and shared by the tests that use them; nobody writes to them"""
    return Case(regime, B, Cin, Cout, H, W, dil, res, relu, tile, amax2, seed)


# ---- the cases of tests/test_gpu_wino_exact.py --------------------------------------------------------------------------------------
# maps: 2 x 9 x 7 is less than one tile per sub-grid at d = 4; 2 x 22 x 38 has its last tile row and column partly outside at every
# dilation; 3 x 36 x 52 at d = 1 is 351 tiles (two GEMM row tiles, the last one padded: rows 351 .. 511 of V are never written)
SMALL, RAGGED, TWO_ROW_TILES = (2, 9, 7), (2, 22, 38), (3, 36, 52)
# (regime, Cin, Cout, (B, H, W), dil, res, relu, amax2)
F4 = [
    # 32 -> 128: k_gemm_f16x3<128,128>
    ('wide', 32, 128, SMALL, 4, True, True, False),
    ('wide', 32, 128, RAGGED, 1, False, False, False),
    ('wide', 32, 128, RAGGED, 2, True, True, False),
    ('planes_w', 32, 128, RAGGED, 1, True, True, False),
    ('planes_w', 32, 128, SMALL, 4, False, False, False),
    ('planes_x', 32, 128, RAGGED, 4, True, True, False),
    ('planes_x', 32, 128, SMALL, 2, False, False, False),
    # 64 -> 384: the 128 tile with three channel tiles
    ('wide', 64, 384, RAGGED, 4, False, True, False),
    ('planes_w', 64, 384, RAGGED, 2, False, True, False),
    ('planes_x', 64, 384, SMALL, 1, True, True, False),
    # 256 -> 256: k_gemm_f16x3_stag<256,256> with float32 V
    ('wide', 256, 256, RAGGED, 4, True, True, False),
    ('wide', 256, 256, TWO_ROW_TILES, 1, False, True, False),
    ('planes_w', 256, 256, SMALL, 4, True, False, False),
    ('planes_x', 256, 256, RAGGED, 2, False, True, False),
    # Cout 512: V written as planes under key 4 = 2
    ('wide', 256, 512, RAGGED, 2, False, True, False),
    ('wide', 256, 512, SMALL, 4, True, False, False),
    ('wide', 512, 512, RAGGED, 4, True, True, False),
    ('wide', 512, 512, RAGGED, 1, False, False, False),
    ('wide', 64, 512, TWO_ROW_TILES, 1, False, True, False),       # the never-written rows as planes
    ('planes_x', 64, 512, RAGGED, 4, True, True, False),           # k_wino4_in<PLANES> with a low plane that counts
    ('planes_w', 64, 512, RAGGED, 1, False, True, False),
    ('planes_x', 256, 512, SMALL, 1, True, True, False),
    ('planes_x', 512, 512, SMALL, 2, False, True, False),
    # the amax word twice the true maximum (the contract is amax >= max |x|): every plane sits one bit lower
    ('planes_x', 64, 512, SMALL, 1, True, True, True),
    ('wide', 256, 256, SMALL, 2, False, True, True),
]
# spa_conv3x3_wino_f32, F(2x2,3x3), 'wide' with w = k: (Cin, Cout, (B, H, W), dil, res, relu); 2 x 22 x 38 at d = 1 is 418 tiles
F2 = [
    (32, 64, SMALL, 4, True, True),
    (32, 128, RAGGED, 1, False, False),
    (64, 192, RAGGED, 2, True, True),
    (256, 256, RAGGED, 4, False, True),
    (512, 512, SMALL, 1, True, False),
]
LARGE = 'w16_256_cin64_res'                   # conv_plan.WINO: at 'full2' every workgroup of the staggered GEMM computes two tiles
MUTANT_LOW = ('planes_w', 32, 128, RAGGED, 1, True, True, False)
MUTANT_TERM = ('wide', 512, 512, RAGGED, 4, True, True, False)


def f4(key):
    regime, Cin, Cout, (B, H, W), dil, res, relu, amax2 = key
    return case(regime, B, Cin, Cout, H, W, dil, res, relu, 4, amax2)


def f2(key):
    Cin, Cout, (B, H, W), dil, res, relu = key
    return case('wide', B, Cin, Cout, H, W, dil, res, relu, 2)


def ident(key):
    return '-'.join('x'.join(str(i) for i in v) if isinstance(v, tuple) else str(int(v)) if isinstance(v, bool) else str(v) for v in key)


def large_case(n_cu, L):
    """the smallest shape conv_plan finds for LARGE at 'full2': (Case, plan); 'wide' only"""
    import conv_plan as cp
    Cin, Cout, dil, res, relu, tile, split = cp.WINO[LARGE]
    B, H, W, p = cp.plan_wino(LARGE, 'full2', n_cu, L)
    return case('wide', B, Cin, Cout, H, W, dil, res, relu, tile), p
