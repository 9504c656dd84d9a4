"""CPU self-check of tests/wino_exact.py, the exact-operand cases behind test_gpu_wino_exact.py: every case meets the premises its
exactness rests on (asserted when the case is made; the figures are printed here), the whole arithmetic of the Winograd kernels
restated in float32 on the CPU — tile decode, gather with zero halo, B^T x B in the header's order, the scaled planes, the three
products in separate accumulators over a shuffled channel order, cs and 2^(e - 14), A^T M A twice, bias, residual, ReLU, clipped
scatter — gives the float64 reference bit for bit, and `check` rejects that restatement with each of the mistakes a tolerance of
1e-5 of the largest output cannot see."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan as cp  # noqa: E402
import wino_exact as we  # noqa: E402

torch = pytest.importorskip('torch')
F = torch.nn.functional


def restate(c, form, seed=1, drop=None, no_low=False, cs_double=None, p_off=None, eighth=0.125, wrap=False, swap_sub=False,
            clip=0, pad_row=False):
    """the layer of Case c as the kernels compute it, in float32 on the CPU; form 'f32' (spa_conv3x3_wino_f32 / _wino4_f32) or
    'f16s' (spa_conv3x3_wino4_f16s).  The mutants as switches: drop = (position, channel): that term missing from every output;
    no_low: the big operand's low plane zeroed; cs_double: that position's cs doubled; p_off: that entry of p = 4 4 4 3 3 4 one
    higher in the scale of V (cs keeps the right one); eighth: the 0.125 of wino4_at; wrap: a halo pixel left or right of the
    image read from the flat address; swap_sub: sx and sy exchanged in the output kernel's tile decode; clip: rows the output
    clipping loses; pad_row: the last tile reads row T of M, the first of the padding"""
    Engine = we.engine()
    tile, n, g = c.tile, c.tile + 2, c.geom
    B, Cin, Cout, H, W = c.shape
    T = g.T
    V = we.transform_in(g.gather(c.x.float(), wrap=wrap), tile)
    assert V.dtype == torch.float32
    Vz = V.reshape(T, n * n, Cin).permute(1, 0, 2).contiguous()
    perm = torch.randperm(Cin, generator=torch.Generator().manual_seed(seed))
    M = torch.ones((n * n, g.Tpad, Cout), dtype=torch.float32)                 # rows T .. Tpad: whatever the GEMM made of stale V
    if form == 'f32':
        U = Engine.winograd_weights(c.w, tile).clone()
        if drop is not None:
            U[drop[0], :, drop[1]] = 0
        for z in range(n * n):
            M[z, :T] = Vz[z][:, perm] @ U[z][:, perm].t()
    else:
        assert tile == 4
        u2, cs = Engine.winograd_weights_split(c.w)
        Uh = u2[:, :, :, 0, :].reshape(36, Cout, Cin).float()
        Ul = u2[:, :, :, 1, :].reshape(36, Cout, Cin).float()
        if drop is not None:
            Uh[drop[0], :, drop[1]] = 0
            Ul[drop[0], :, drop[1]] = 0
        if no_low and c.regime == 'planes_w':
            Ul = torch.zeros_like(Ul)
        e = we.amax_exp(c.amax_word)
        p = list(we.P4)
        if p_off is not None:
            p[p_off] += 1
        for z in range(36):
            vs = Vz[z] * torch.tensor(2.0 ** (14 - e - we.psum(z, p)), dtype=torch.float32)
            h = vs.half().float()
            l = (vs - h).half().float()
            if no_low and c.regime == 'planes_x':
                l = torch.zeros_like(l)
            lh = l[:, perm] @ Uh[z][:, perm].t()
            hl = h[:, perm] @ Ul[z][:, perm].t()
            hh = h[:, perm] @ Uh[z][:, perm].t()                                  # (l.l is dropped by design)
            scale = torch.tensor(float(cs[z]) * (2.0 if cs_double == z else 1.0), dtype=torch.float32) * torch.tensor(2.0 ** (e - 14), dtype=torch.float32)
            M[z, :T] = scale * ((lh + hl) + hh)
    rows = torch.arange(T)
    if pad_row:
        rows[-1] = T
    m = M[:, rows].permute(1, 0, 2).reshape(T, n, n, Cout)
    o = we.transform_out(m, tile, eighth)
    assert o.dtype == torch.float32
    gout = we.Geom(B, H, W, c.dil, tile, swap_sub=swap_sub)
    v = gout.scatter(o, clip_rows=clip, strict=not (swap_sub or clip))
    v = v + c.bias.float().view(1, -1, 1, 1)
    if c.res is not None:
        v = v + c.res.float()
    return torch.relu(v) if c.relu else v


def _lib():
    import importlib
    return importlib.import_module('superpixel-align_amd')._lib.lib()


def _show(name, c):
    print('%-44s T %4d  ' % (name, c.geom.T) + '  '.join('%s %.2f' % kv for kv in c.bounds.items()))


def test_every_case_meets_its_premises_and_bound():
    """the premises (a) .. (f) are asserted when a case is made; here every case of the GPU file is made, its figures are printed,
    the Winograd route in float64 is the reference, and the regime is what it says"""
    n = 0
    cases = [(we.ident(k), we.f4(k)) for k in we.F4] + [('F(2x2) ' + we.ident(k), we.f2(k)) for k in we.F2]
    cases.append(('large ' + we.LARGE, we.large_case(256, _lib())[0]))
    for name, c in cases:
        _show(name, c)
        assert c.bounds and all(b < 24 for k, b in c.bounds.items() if k != 'low share')
        if c.regime != 'wide':
            assert c.bounds['low share'] >= we.LOW_SHARE
            assert ('h.l' in c.bounds) == (c.regime == 'planes_w') and ('l.h' in c.bounds) == (c.regime == 'planes_x')
        else:
            assert 'h.l' not in c.bounds and 'l.h' not in c.bounds
        ref = c.ref()
        pre = c.pre64()
        assert bool((pre < 0).any()) and bool((pre > 0).any())
        conv = pre - c.bias.view(1, -1, 1, 1) - (c.res if c.res is not None else 0)
        assert torch.equal(c.scatter_exact(), conv), 'the Winograd route in float64 is not the convolution'
        assert torch.equal(conv, (225 if c.tile == 4 else 1) * F.conv2d(c.x, c.k, None, 1, c.dil, c.dil))
        assert float(c.x.abs().max()) == float(c.x.view(-1)[0]) and ref.dtype == torch.float32
        n += 1
    assert n == len(we.F4) + len(we.F2) + 1


def test_the_cases_reach_the_mechanisms_they_are_for():
    L = _lib()
    pairs = {(k[0], k[1], k[2]) for k in we.F4}
    assert {('wide', 32, 128), ('wide', 256, 256), ('wide', 256, 512), ('wide', 512, 512), ('wide', 64, 384)} <= pairs
    for regime in ('planes_w', 'planes_x'):
        assert {(32, 128), (64, 384), (256, 256), (64, 512)} <= {(k[1], k[2]) for k in we.F4 if k[0] == regime}
        assert {k[4] for k in we.F4 if k[0] == regime} == {1, 2, 4}
    assert {k[4] for k in we.F4 if k[0] == 'wide'} == {1, 2, 4} and {k[3] for k in we.F2} == {1, 2, 4}
    assert {(k[5], k[6]) for k in we.F4} == {(r, a) for r in (False, True) for a in (False, True)}
    assert sum(k[7] for k in we.F4) == 2
    # the maps: less than one tile per sub-grid; last tile row and column partly outside; two GEMM row tiles, the last one padded
    g = we.Geom(*we.SMALL, 4, 4)
    assert (g.th, g.tw, g.T) == (1, 1, 32)
    for d in (1, 2, 4):
        g = we.Geom(*we.RAGGED, d, 4)
        hs, ws = -(-22 // d), -(-38 // d)
        assert hs % 4 and ws % 4 and g.th * 4 > hs and g.tw * 4 > ws
        assert g.Tpad == int(L.spa_wino4_tiles(*we.RAGGED, d))
    g = we.Geom(*we.TWO_ROW_TILES, 1, 4)
    assert (g.T, g.Tpad) == (351, 512) and any(k[3] == we.TWO_ROW_TILES and k[2] == 512 for k in we.F4)
    g = we.Geom(*we.RAGGED, 1, 2)
    assert (g.T, g.Tpad) == (418, 512) and g.Tpad == int(L.spa_wino_tiles(*we.RAGGED, 1))
    # the interleaved numbering runs at dilation 4: the restated decode is the library's, tile by tile
    out = (ctypes.c_int32 * 5)()
    g = we.Geom(*we.RAGGED, 4, 4)
    for t in range(g.T):
        assert L.spa_wino4_tile_decode(*we.RAGGED, 4, 1, t, out) == 0
        assert tuple(out) == (int(g.b[t]), int(g.sy[t]), int(g.sx[t]), int(g.ty[t]), int(g.tx[t]))
    # the planned shape: every workgroup of the staggered GEMM ends at its second tile
    c, p = we.large_case(256, L)
    assert p['kernel'] == 'k_gemm_f16x3_stag<256,256>' and p['slots'] < p['tiles'] <= 2 * p['slots'] and c.regime == 'wide'
    assert c.geom.Tpad == p['rows'] and cp.TARGETS[1] == 'full2'


def test_per_tap_reference_is_the_convolution():
    """`taps64`, the reference of the large shape, held to F.conv2d: the same float64 integers"""
    for key in (we.F4[0], we.F4[3], we.F4[13]):
        c = we.f4(key)
        assert torch.equal(c.ref('cpu', taps=True), c.ref())


RESTATED = [(we.F4[i], form) for i in (0, 3, 5, 8, 9, 10, 16, 19, 23, 24) for form in ('f16s', 'f32')] + [(k, 'f32') for k in (we.F2[0], we.F2[2], we.F2[4])]


@pytest.mark.parametrize('key,form', RESTATED, ids=lambda v: we.ident(v) if isinstance(v, tuple) else v)
def test_restated_arithmetic_is_the_reference_bit_for_bit(key, form):
    c = we.f4(key) if len(key) == 8 else we.f2(key)
    we.check(restate(c, form), c.ref(), 'restatement')
    if form == 'f16s':
        we.check(restate(c, form, seed=2), c.ref(), 'another channel order')


def _rejected(c, form, **kw):
    with pytest.raises(AssertionError, match='outputs differ'):
        we.check(restate(c, form, **kw), c.ref(), str(kw))


def test_one_dropped_term_at_512_channels_fails_the_exact_check():
    """512 -> 512, K = 4608: ONE (channel, position) term of the 36 x 512 missing from every output"""
    c = we.f4(we.MUTANT_TERM)
    assert c.shape[1] == 512
    for form in ('f16s', 'f32'):
        we.check(restate(c, form), c.ref())
        _rejected(c, form, drop=(22, 137))
        _rejected(c, form, drop=(0, 511))


@pytest.mark.parametrize('key', [we.MUTANT_LOW, we.F4[5], we.F4[19]], ids=we.ident)
def test_a_zeroed_low_plane_fails_the_exact_check(key):
    c = we.f4(key)
    we.check(restate(c, 'f16s'), c.ref())
    _rejected(c, 'f16s', no_low=True)


@pytest.mark.parametrize('key', [we.F4[5], we.F4[10], we.F4[3]], ids=we.ident)
def test_check_rejects_every_mutant(key):
    """dilation-4 ragged maps in 'planes_x' and 'wide', a dilation-1 one in 'planes_w'"""
    c = we.f4(key)
    we.check(restate(c, 'f16s'), c.ref())
    mutants = {"one position's cs doubled": dict(cs_double=21), 'p = 4 4 4 3 3 4 with one entry off by one': dict(p_off=3),
               '0.125 -> 0.25 in wino4_at': dict(eighth=0.25), 'a halo pixel from the wrapped address': dict(wrap=True),
               "the last partial tile's clipping off by one row": dict(clip=1), 'a padding row of M in place of a tile': dict(pad_row=True)}
    if c.dil == 4:
        mutants['sx and sy exchanged in the tile decode'] = dict(swap_sub=True)
    for name, kw in mutants.items():
        with pytest.raises(AssertionError, match='outputs differ'):
            we.check(restate(c, 'f16s', **kw), c.ref(), name)
    for kw in (dict(eighth=0.25), dict(wrap=True), dict(pad_row=True)):
        _rejected(c, 'f32', **kw)
