"""CPU self-check of tests/conv_plan.py, the tile plans behind test_gpu_conv_persistent.py: on a 256-CU MI355X every case's shape
gets the kernel it is meant for and lands at its target — one tile past a round, exactly two rounds, three rounds less one —
as closely as the launcher's tile granularity allows.  A launcher change that moves a case away from its target fails here."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_plan as cp  # noqa: E402

N_CU = 256               # MI355X


def _check(B, H, W, p, granularity=8):
    assert B >= 2
    assert p['slots'] > 0 and p['miss'] >= 0
    assert p['miss'] < granularity, cp.describe(B, H, W, p)
    t, s = p['tiles'], p['slots']
    if p['target'] == 'wrap':
        assert s < t
    elif p['target'] == 'full2':
        assert s < t <= 2 * s
    else:
        assert 2 * s < t < 3 * s


def test_small_plans_by_hand():
    # the formulas against counts worked out from the launchers
    p = cp.conv_f32(N_CU, 2, 9, 300, 64, 128)                      # 128 x 128 tiles, 64 KB of LDS: two per CU
    assert (p['tiles'], p['slots'], p['bn'], p['per_cu']) == (2 * 9 * 3, 54, 128, 2)
    p = cp.conv_f32(N_CU, 30, 64, 512, 64, 64, split=True)        # the 64 -> 64 layer of 30 images: k_conv3x3_p16
    assert p['kernel'] == 'k_conv3x3_p16<64,256>' and (p['tiles'], p['slots']) == (30 * 64 * 2, 256)
    p = cp.conv_f32(N_CU, 1, 3, 1000, 32, 64, split=True)          # 1000 of 1024 pixels: the 512-pixel split tile
    assert p['bn'] == 512 and p['per_cu'] == 1 and p['tiles'] == 6
    p = cp.gemm_f16x3(N_CU, 61440, 512, 512)                       # the D-22 Winograd GEMM at B = 30: ~8 600 tiles for 256
    assert p['kernel'] == 'k_gemm_f16x3_stag<256,256>' and p['tiles'] == 240 * 2 * 36 and p['slots'] == 256
    p = cp.conv_bf16_light(N_CU, 2, 64, 640, 64, 128, 9, 1)        # 73 728 bytes of weights: two per CU, two channel blocks
    assert (p['mi'], p['nblk'], p['per_cu'], p['tiles']) == (4, 2, 2, 2 * 64 * 10)
    assert p['grid'] == (160, 2)


@pytest.mark.parametrize('target', cp.TARGETS)
def test_plans_reach_their_targets(target):
    for name, case in cp.DIRECT.items():
        B, H, W, p = cp.plan_direct(name, target, N_CU)
        _check(B, H, W, p)
        if name.startswith('p16'):
            assert p['kernel'].startswith('k_conv3x3_p16'), name
        else:
            assert p['kernel'].startswith('k_conv3x3_f32<%d,%d,' % (p['bm'], case[2])), name
        if case[6] == 'pred':
            assert ',split' in p['kernel']
        for k, v in case[7].items():
            assert p[k] == v, name
        assert W % p['bn'] != 0 or case[2] == 1
    for name in cp.STRIDE2:
        _check(*cp.plan_stride2(name, target, N_CU))
    for name in cp.SMALL:
        _check(*cp.plan_small(name, target, N_CU))
    _check(*cp.plan_layer2(target, N_CU))
    for name in cp.LIGHT:
        B, H, W, p = cp.plan_light(name, target, N_CU)
        assert p['nblk'] > 1 and p['grid'][0] * p['nblk'] >= N_CU
        # (with several channel blocks the launcher halves the x-grid of a capped launch: 'wrap' lands near two passes)
        _check(B, H, W, p, granularity=p['slots'] if target == 'wrap' else 10)


@pytest.mark.parametrize('target', cp.TARGETS)
def test_winograd_plans_reach_their_targets(spa, target):
    L = spa._lib.lib()
    for name, (Cin, Cout, dil, res, relu, tile, split) in cp.WINO.items():
        B, H, W, p = cp.plan_wino(name, target, N_CU, L)
        assert p['rows'] % 256 == 0
        # a count is 36 (16) problems x row tiles x channel tiles: the granularity of the target
        g = (36 if tile == 4 else 16) * (Cout // p['bm']) * (256 // p['bn'])
        _check(B, H, W, p, granularity=g)
        if split:
            assert p['kernel'] == ('k_gemm_f16x3_stag<256,256>' if Cout % 256 == 0 else 'k_gemm_f16x3<128,128>')
