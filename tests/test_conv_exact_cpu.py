"""CPU self-check of tests/conv_exact.py, the exact-operand cases behind test_gpu_conv_exact.py: every case meets the bound its
exactness rests on, the arithmetic of each regime restated in torch (float32 accumulation, one rounding; for the plane regimes
h = rn16, l = rn16(rest), three products) gives the reference bit for bit, and `check` rejects that restatement with each of the
mistakes the tolerance tests cannot see."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact as ce  # noqa: E402
import conv_plan as cp  # noqa: E402

torch = pytest.importorskip('torch')
F = torch.nn.functional


def _truncate_to_bf16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def _wrapped_padding(x, d):
    """zero padding of d pixels whose left / right border columns hold the neighbouring row's pixels instead: what flat address
    arithmetic reads when the column is not bounded (pixel (y, W + j) is pixel (y + 1, j) of a row-major image)"""
    B, C, H, W = x.shape
    xp = F.pad(x, (d, d, d, d))
    n = min(d, W)
    xp[:, :, d:d + H - 1, d + W:d + W + n] = x[:, :, 1:, :n]
    xp[:, :, d + 1:d + H, d - n:d] = x[:, :, :H - 1, W - n:]
    return xp


def restate(c, dtype, drop=None, wrap=False, swap=None, truncate=False, no_low=False, move_image=False):
    """the convolution of Case c as the kernels compute it, in torch on the CPU, with the mutants as switches
    drop = (channel, ky, kx): that term missing from every output; wrap: border taps read the neighbouring row; swap = (c0, c1):
    two input channels exchanged in the weights only; truncate: bf16 by truncation; no_low: the low plane zeroed; move_image: image 0's
    output written at image 1's position and the other way round"""
    x, w = c.x.float(), c.w.float().clone()
    if drop is not None:
        w[:, drop[0], drop[1], drop[2]] = 0
    if swap is not None:
        w[:, [swap[0], swap[1]]] = w[:, [swap[1], swap[0]]]
    pad = c.dil if c.taps == 9 else 0
    if wrap:
        assert c.stride == 1 and c.taps == 9
        x, pad = _wrapped_padding(x, c.dil), 0

    def conv(a, b):
        return F.conv2d(a, b, None, c.stride, pad, c.dil)                 # float32 accumulation
    if c.regime.startswith('planes'):
        hx, lx, sx = ce.split(x)
        hw, lw, sw = ce.split(w)
        if no_low:
            lx, lw = torch.zeros_like(lx), torch.zeros_like(lw)
        acc = conv(hx, lw)
        acc = acc + conv(lx, hw)
        acc = acc + conv(hx, hw)                                          # (l l is dropped by design)
        v = acc * torch.tensor(1.0 / (sx * sw), dtype=torch.float32)
    else:
        v = conv(x, w)
    v = v + c.bias.float().view(1, -1, 1, 1)
    if c.res is not None:
        v = v + c.res.float()
    if c.relu:
        v = torch.relu(v)
    assert v.dtype == torch.float32
    y = _truncate_to_bf16(v) if truncate else v.to(dtype)
    if move_image:
        y = y.flip(0)
    return y


def test_every_gpu_case_meets_its_bound_and_condition():
    n = 0
    for name, c in ce.all_cases():
        assert c.bound < ce.LIMIT                                       # (asserted by the generator too)
        y, y2 = c.ref64()
        assert torch.equal(y, y.round()) and float(y.abs().max()) < ce.LIMIT
        if c.regime == 'unit':
            assert c.unit_fraction() >= 0.99, (name, c.K, c.unit_fraction())
        if c.regime == 'wide' and c.relu and name in ('bf16', 'light'):
            pre = F.conv2d(c.x, c.w, c.bias, c.stride, c.dil if c.taps == 9 else 0, c.dil)
            assert bool((pre < 0).any()) and bool((pre > 0).any())      # both signs reach the ReLU
        n += 1
    assert n == 2 * (len(ce.BF16) + len(ce.LIGHT)) + 2 * (len(ce.F16S_3X3) + len(ce.F16S_1X1) + len(ce.S2)) + 3 + len(ce.WIDE_SMALL) + 1


def test_wide_regime_exercises_the_bf16_rounding_and_its_ties():
    c = ce.case('wide', 1, 512, 512, 6, 40, 9, 1, 4, False, True)
    y = c.ref64()[0]
    assert float(y.max()) > 1000
    inexact = y.float().to(torch.bfloat16).double() != y
    # a tie: the exact integer lies half way between two bf16 neighbours (an odd multiple of half the spacing at its magnitude)
    spacing = torch.exp2(torch.floor(torch.log2(y.clamp_min(1))) - 7)
    tie = inexact & (torch.remainder(y, spacing) == spacing / 2)
    print("rounded %.3f, ties %.3f of all outputs" % (float(inexact.double().mean()), float(tie.double().mean())))
    assert float(inexact.double().mean()) > 0.1                # (the ReLU holds half of the outputs at zero)
    assert 0.05 < float(tie.double().mean()) < 0.3


def test_the_cases_reach_the_branches_they_are_for():
    # spa_conv3x3_bf16: the `rem` branch of the XCD remap, several channel tiles, all three tiles with and without the residual
    tiles = {(ce.bf16_tiles(B, Cin, Cout, H, W)[0], res) for B, Cin, Cout, H, W, dil, res, relu in ce.BF16}
    assert tiles == {(bm, r) for bm in (64, 128, 256) for r in (False, True)}
    B, Cin, Cout, H, W = ce.BF16[0][:5]
    assert ce.bf16_tiles(B, Cin, Cout, H, W) == (256, 2, 12)
    assert any(ce.bf16_tiles(*k[:5])[1] == 3 for k in ce.BF16)
    assert {k[5] for k in ce.BF16} == {1, 2, 3, 4} and any(k[1] == 512 for k in ce.BF16)
    assert {k[4] for k in ce.BF16} >= {255, 256, 257} and any(k[3] == 1 for k in ce.BF16)
    # spa_conv_bf16_light: every instantiation the dispatch of csrc/spa_convl.hip has, once
    got = sorted((Cin, taps, s, cp.light_mi(Cin, Cout, taps)) for Cin, Cout, taps, s, dil, res, relu, B, H, W in ce.LIGHT)
    want = [(c, t, s, m) for c, m in ((32, 4), (64, 4), (16, 2), (32, 2), (16, 1)) for t in (9, 1) for s in (1, 2)]
    want += [(c, 1, s, m) for c in (128, 256) for m in (4, 8) for s in (1, 2)]
    assert got == sorted(want) and len(set(got)) == len(got) == 28
    assert any(k[0] == 64 and k[4] == 2 for k in ce.LIGHT)
    assert {k[5] for k in ce.LIGHT} == {False, True} and {k[6] for k in ce.LIGHT} == {False, True}
    # the split-plane forms: k_conv3x3_p16 is selectable at every 3x3 case, the 2-D tile kernel at every stride-2 case
    for B, C, H, W, dil, res, relu in ce.F16S_3X3:
        assert cp.conv_f32(256, B, H, W, C, C, split=True)['kernel'].startswith('k_conv3x3_p16')
    assert {(k[1], k[4]) for k in ce.F16S_3X3} == {(c, d) for c in (64, 128) for d in (1, 2, 4)}
    assert {k[3] for k in ce.F16S_3X3} == {5, 257}
    assert all(Cin in (32, 64) and Cout in (64, 128) for B, Cin, Cout, Hi, Wi in ce.S2)


SMALL = [('unit', 2, 64, 64, 9, 20, 9, 1, 4, True, True), ('wide', 2, 64, 64, 9, 20, 9, 1, 4, True, True),
         ('planes_x', 2, 64, 64, 9, 20, 9, 1, 4, True, True), ('planes_w', 2, 128, 128, 9, 20, 9, 1, 4, False, False),
         ('unit', 2, 32, 64, 9, 21, 9, 2, 1, False, True), ('wide', 2, 128, 192, 5, 33, 1, 1, 1, True, False),
         ('planes_w', 2, 256, 512, 3, 11, 1, 1, 1, False, True)]
LARGE_K = [('unit', 1, 512, 512, 6, 40, 9, 1, 4, False, True), ('wide', 1, 512, 512, 6, 40, 9, 1, 4, False, True)]


def _dtype(c):
    return torch.float32 if c.regime.startswith('planes') else torch.bfloat16


@pytest.mark.parametrize('key', SMALL + LARGE_K, ids=lambda k: '-'.join(str(v) for v in k))
def test_restated_arithmetic_is_the_reference_bit_for_bit(key):
    """float32 accumulation in whatever order the CPU convolution takes, one rounding: the float64 reference's bits"""
    c = ce.case(*key)
    ce.check(restate(c, _dtype(c)), c.ref(_dtype(c))[0], 'restatement')


@pytest.mark.parametrize('key', LARGE_K, ids=lambda k: k[0])
def test_one_dropped_term_at_512_channels_fails_the_exact_check(key):
    """a 512 -> 512 layer (K = 4608) that leaves one (channel, tap) term out of EVERY output: an error of one term of the sum, the size
    a tolerance relative to the largest output is loosest against; `check` rejects it, and in the unit regime every output whose tap
    lies inside the image shows it"""
    c = ce.case(*key)
    ref = c.ref(torch.bfloat16)[0]
    y = restate(c, torch.bfloat16, drop=(137, 0, 2))
    with pytest.raises(AssertionError, match='outputs differ'):
        ce.check(y, ref)
    if c.regime == 'unit':
        # dilation 4, tap (ky 0, kx 2): rows 4.., columns ..35; only what the ReLU holds at zero either way stays the same
        pre = F.conv2d(c.x, c.w, c.bias, 1, 4, 4)
        changed = (y != ref)
        inside = torch.zeros_like(changed)
        inside[:, :, 4:, :36] = True
        assert not bool((changed & ~inside).any())
        assert bool(changed[inside & (pre > 1)].all())


@pytest.mark.parametrize('key', SMALL[:4], ids=lambda k: k[0])
def test_check_rejects_every_mutant(key):
    c = ce.case(*key)
    dt = _dtype(c)
    ref = c.ref(dt)[0]
    ce.check(restate(c, dt), ref)
    mutants = {'dropped term': dict(drop=(5, 2, 0)), 'border tap reads the neighbouring row': dict(wrap=True),
               'input channels exchanged in the weights': dict(swap=(3, 40)), 'image written at another position': dict(move_image=True)}
    if c.regime == 'wide':
        mutants['truncation'] = dict(truncate=True)
    if c.regime.startswith('planes'):
        mutants['low plane zeroed'] = dict(no_low=True)
    for name, kw in mutants.items():
        with pytest.raises(AssertionError, match='outputs differ'):
            ce.check(restate(c, dt, **kw), ref, name)


def test_check_reports_the_first_difference():
    c = ce.case(*SMALL[0])
    ref = c.ref(torch.bfloat16)[0]
    y = ref.clone()
    y[1, 7, 3, 2] += 1
    y[1, 9, 0, 0] += 1
    with pytest.raises(AssertionError) as e:
        ce.check(y, ref, 'probe')
    msg = str(e.value)
    assert 'probe: 2 of %d outputs differ' % ref.numel() in msg and '(1, 7, 3, 2)' in msg
    with pytest.raises(AssertionError):
        ce.check(ref.float(), ref)                       # the type is part of the answer
