"""Tile plans of libspalign's persistent convolution launchers: how many output tiles a call has and how many workgroups the
launcher starts for them, restated from the launchers (csrc/spa_conv32.hip, spa_convp.hip, spa_gemm16.hip, spa_convs.hip,
spa_stem.hip, spa_convl.hip), and a search for shapes whose tile count lands at a chosen place relative to the grid.

Every plan is a dict with 'tiles' (work units of the persistent loop, all problems of a z-batched launch together), 'slots'
(units the grid takes per round: the workgroup count, or 4 x it for the light kernel whose four waves take a strip each),
'grid' (the launch grid, x and y) and the tile geometry.  Nothing here touches a GPU: the Winograd forms take the row count
from a callable (spa_wino4_tiles / spa_wino_tiles of the library, host functions).

Targets (`pick`):
    'wrap'    tiles = slots + 1 — one workgroup takes a second tile
    'full2'   tiles = 2 slots   — every workgroup ends at its second tile, nothing is staged after the last one
    'ragged'  tiles = 3 slots - 1 — three rounds, the last one ragged
A product B x rows x x-tiles x channel tiles (x 36 problems for the Winograd GEMMs) cannot hit every count (slots + 1 = 257
is prime), so `pick` returns the closest count on the target's side: above slots for 'wrap', at most 2 slots for 'full2',
between 2 slots and 3 slots - 1 for 'ragged'; 'miss' is the distance.
"""
import functools

C32_HALO = 4
KIB = 1024


def conv_f32(n_cu, B, H, W, Cin, Cout, taps=9, split=False, convp=True, zcount=1):
    """conv_f32_launch (spa_conv32.hip): spa_conv3x3_f32 / spa_conv1x1_f32, spa_conv3x3_f16s / spa_conv1x1_f16s (split) and the
    float32 Winograd GEMMs (zcount 16 / 36).  convp: the planes-in-LDS kernel is selectable (spa_debug_set(ctx, 1, 1))."""
    if split and convp and taps == 9 and Cout in (64, 128) and Cin >= 64 and zcount == 1:
        return conv3x3_p16(n_cu, B, H, W, Cin, Cout)
    bm = 256 if Cout % 256 == 0 else (128 if Cout % 128 == 0 else 64)
    wide64 = split and bm == 64 and (W + 255) // 256 * 256 * 4 <= 5 * W
    wide512 = split and bm == 64 and taps == 9 and (W + 511) // 512 * 512 * 4 <= 5 * W
    bn = 512 if wide512 else (256 if bm == 256 or wide64 else 128)
    xtiles, ntiles = (W + bn - 1) // bn, Cout // bm
    total = B * H * xtiles * ntiles
    lds = 2 * bm * 128 + 2 * (bn + 2 * C32_HALO) * 128
    per_cu = 1 if lds > 80 * KIB else (2 if lds > 53 * KIB or (split and bm == 64) else 3)
    grid = min(n_cu * per_cu, total * zcount)
    name = 'k_conv3x3_f32<%d,%d,%d%s>' % (bm, taps, bn, ',split' if split else '')
    return dict(kernel=name, tiles=total * zcount, slots=grid, grid=(grid, 1), bm=bm, bn=bn, nk=taps * (Cin // 32), per_cu=per_cu)


def conv_s2(n_cu, B, Hi, Wi, Cin, Cout, split=True):
    """spa_conv3x3_s2_f16s (split) / spa_conv3x3_s2_f32: the stride-2 openers, 128-pixel tiles of the output"""
    H, W = (Hi + 1) // 2, (Wi + 1) // 2
    bm, bn = (256 if Cout % 256 == 0 else 128), 128
    xtiles, ntiles = (W + bn - 1) // bn, Cout // bm
    total = B * H * xtiles * ntiles
    lds = 2 * bm * 128 + 2 * (2 * bn + 2 * C32_HALO + (8 if split else 0)) * 128
    per_cu = 1 if lds > 80 * KIB else (2 if lds > 53 * KIB else 3)
    grid = min(n_cu * per_cu, total)
    return dict(kernel='k_conv3x3_f32<%d,9,128,%s,S=2>' % (bm, 'split' if split else 'f32'), tiles=total, slots=grid, grid=(grid, 1),
                bm=bm, bn=bn, nk=9 * (Cin // 32), per_cu=per_cu)


def conv3x3_p16(n_cu, B, H, W, Cin, Cout):
    """conv3x3_p16_launch (spa_convp.hip): one workgroup per CU"""
    bm, bn = Cout, (128 if Cout == 128 else 256)
    total = B * H * ((W + bn - 1) // bn)
    grid = min(n_cu, total)
    return dict(kernel='k_conv3x3_p16<%d,%d>' % (bm, bn), tiles=total, slots=grid, grid=(grid, 1), bm=bm, bn=bn, nk=9 * (Cin // 32), per_cu=1)


def gemm_f16x3(n_cu, rows, Cin, Cout):
    """gemm_f16x3_raw (spa_gemm16.hip): the 36 GEMMs of spa_conv3x3_wino4_f16s, rows = spa_wino4_tiles(B, H, W, dilation)"""
    bm = 256 if Cout % 256 == 0 else 128
    bn = 256 if bm == 256 else 128
    total = rows // bn * (Cout // bm) * 36
    per_cu = 1 if 2 * (bm + bn) * 128 > 80 * KIB else 2
    grid = min(n_cu * per_cu, total)
    name = 'k_gemm_f16x3_stag<256,256>' if bm == 256 else 'k_gemm_f16x3<128,128>'
    return dict(kernel=name, tiles=total, slots=grid, grid=(grid, 1), bm=bm, bn=bn, nk=Cin // 32, per_cu=per_cu)


def conv_small(n_cu, B, H, W, stride):
    """spa_conv_small_f16s (spa_convs.hip): 32 x 8 output tiles (32 x 4 at stride 2), grid 2 x CUs"""
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    TH = 4 if stride == 2 else 8
    total = (Wo + 31) // 32 * ((Ho + TH - 1) // TH) * B
    grid = min(2 * n_cu, total)
    return dict(kernel='k_conv_small_f16x3', tiles=total, slots=grid, grid=(grid, 1), th=TH, tw=32)


def drn_layer2(n_cu, B, H, W):
    """spa_drn_layer2_f16s (spa_stem.hip): 32 x 4 output tiles, grid 3 x CUs"""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    total = (Wo + 31) // 32 * ((Ho + 3) // 4) * B
    grid = min(3 * n_cu, total)
    return dict(kernel='k_drn_layer2_f16x3', tiles=total, slots=grid, grid=(grid, 1), th=4, tw=32)


def light_mi(Cin, Cout, taps):
    """spa_conv_bf16_light: output channels per workgroup / 16"""
    if taps == 1 and Cin >= 128 and Cout % 128 == 0:
        return 8
    if Cout % 64 == 0 and Cin >= 32:
        return 4
    if Cout % 32 == 0 and Cin <= 32:
        return 2
    return 1 if Cin == 16 and Cout % 16 == 0 else 0


def conv_bf16_light(n_cu, B, H, W, Cin, Cout, taps, stride):
    """conv_bf16_light_launch (spa_convl.hip): strips of 64 output pixels, one per wave, 4 per workgroup and pass, grid (gx, nblk)"""
    mi = light_mi(Cin, Cout, taps)
    kstep = 32 if Cin >= 32 else 16
    lds = taps * (Cin // kstep) * mi * 64 * (16 if kstep == 32 else 8)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    nstrips = B * Ho * ((Wo + 63) // 64)
    per_cu = (160 * KIB) // max(lds, 20 * KIB) if lds else 8
    gx = min(n_cu * max(per_cu, 1), (nstrips + 3) // 4)
    nblk = Cout // (16 * mi)
    if nblk > 1:
        gx = max((gx + nblk - 1) // nblk, 1)
    # (gx is capped by the strip groups BEFORE it is divided by nblk: a launch with several channel blocks gives every workgroup
    # about two passes even when one would take all strips, so 'wrap' lands near 2 slots there)
    full = gx * nblk >= n_cu                         # every CU has a workgroup: a shape that says something about the loop
    return dict(kernel='k_conv_bf16_light<%d,%d,%d,%d>' % (Cin, taps, stride, mi), tiles=nstrips, slots=4 * gx, grid=(gx, nblk),
                mi=mi, nblk=nblk, per_cu=per_cu, full=full)


TARGETS = ('wrap', 'full2', 'ragged')


def miss(target, tiles, slots):
    """distance of a tile count from the target, None when it is on the wrong side"""
    if target == 'wrap':
        return tiles - (slots + 1) if tiles > slots else None
    if target == 'full2':
        return 2 * slots - tiles if slots < tiles <= 2 * slots else None
    return 3 * slots - 1 - tiles if 2 * slots < tiles <= 3 * slots - 1 else None


def _xwidths(bns, xtiles_max):
    """widths whose last x-tile is partial: a few pixels short of full, and half full"""
    out = set()
    for bn in bns:
        for xt in range(1, xtiles_max + 1):
            out.add((xt - 1) * bn + bn - 37)
            out.add((xt - 1) * bn + bn // 2 + 5)
    return sorted(w for w in out if w > 8)


@functools.lru_cache(maxsize=None)
def _search(target, plan_key, n_cu, Bs, Hs, Ws, want):
    fn, kw = PLAN_FORMS[plan_key]
    best = None
    for B in Bs:
        for H in Hs:
            for W in Ws:
                p = fn(n_cu, B, H, W, **dict(kw))
                if any(p.get(k) != v for k, v in want):
                    continue
                m = miss(target, p['tiles'], p['slots'])
                if m is None:
                    continue
                key = (m, B * H * W, B)
                if best is None or key < best[0]:
                    best = (key, B, H, W, p)
    assert best is not None, (target, plan_key)
    (m, _, _), B, H, W, p = best
    return B, H, W, dict(p, miss=m, target=target)


PLAN_FORMS = {}


def form(key, fn, **kw):
    PLAN_FORMS[key] = (fn, tuple(sorted(kw.items())))
    return key


def pick(target, key, n_cu, dil=1, bns=(128,), xtiles_max=48, Bmax=64, want=(), Hi_min=None):
    """(B, H, W, plan) of the smallest shape (B >= 2, H a few rows above 2 x dil, the last x-tile partial) whose tile count is
    closest to the target; want: plan entries the shape must have (e.g. bn = 512)"""
    h0 = Hi_min if Hi_min is not None else 2 * dil + 1
    return _search(target, key, n_cu, tuple(range(2, Bmax + 1)), tuple(range(h0, h0 + 8)), tuple(_xwidths(bns, xtiles_max)),
                   tuple(sorted(dict(want).items())))


def pick_wino(target, n_cu, rows_fn, Cin, Cout, dil, gemm=gemm_f16x3, zcount=36):
    """(B, H, W, plan) for the Winograd GEMMs: rows = rows_fn(B, H, W, dil) (the library's spa_wino4_tiles / spa_wino_tiles)"""
    best = None
    for B in range(2, 17):
        for H in range(2 * dil + 1, 2 * dil + 9):
            for W in range(17, 600, 6):
                rows = int(rows_fn(B, H, W, dil))
                if gemm is gemm_f16x3:
                    p = gemm_f16x3(n_cu, rows, Cin, Cout)
                else:
                    p = conv_f32(n_cu, 1, rows // 256, 256, Cin, Cout, taps=1, zcount=zcount)
                p['rows'] = rows
                m = miss(target, p['tiles'], p['slots'])
                if m is None:
                    continue
                key = (m, B * H * W, B)
                if best is None or key < best[0]:
                    best = (key, B, H, W, dict(p, miss=m, target=target))
    assert best is not None
    return best[1:]


def describe(B, H, W, p):
    g = p['grid']
    return '%s: B %d H %d W %d -> %d tiles (%s %d: miss %d), grid %d x %d (%d per round), %.2f rounds' % (
        p['kernel'], B, H, W, p['tiles'], p['target'], {'wrap': p['slots'] + 1, 'full2': 2 * p['slots'],
                                                        'ragged': 3 * p['slots'] - 1}[p['target']], p['miss'],
        g[0], g[1], p['slots'], p['tiles'] / p['slots'])


# ---- the cases of tests/test_gpu_conv_persistent.py and their plans ---------------------------------------------------------------
# name: (Cin, Cout, taps, dil, res, relu, path); path 'f32' = spa_conv3x3_f32 / spa_conv1x1_f32, 'f16s' = spa_conv3x3_f16s /
# spa_conv1x1_f16s (k_conv3x3_p16 where it applies), 'pred' = spa_conv3x3_f16s with k_conv3x3_p16 switched off
# (spa_debug_set(ctx, 1, 0)); want: the tile the shape must get
DIRECT = {
    'f32_64x9_cin32_d1_res': (32, 64, 9, 1, True, True, 'f32', {}),                # nk 9 (odd): the parities flip per tile
    'f32_128x9_cin96_d3': (96, 128, 9, 3, False, False, 'f32', {}),
    'f32_256x9_cin64_d2_res': (64, 256, 9, 2, True, True, 'f32', {}),
    'f32_64x9_cin64_d4': (64, 64, 9, 4, False, True, 'f32', {}),
    'f32_128x1_cin32_res': (32, 128, 1, 1, True, False, 'f32', {}),                # nk 1: the only K step stages the next tile
    'f32_256x1_cin160': (160, 256, 1, 1, False, True, 'f32', {}),                  # nk 5
    'f32_64x1_cin96': (96, 64, 1, 1, False, False, 'f32', {}),                     # nk 3
    'f16s_64x9_cin32_bn512_res': (32, 64, 9, 1, True, True, 'f16s', {'bn': 512}),  # the 512-pixel split tile
    'f16s_64x9_cin32_bn256_d3': (32, 64, 9, 3, False, True, 'f16s', {'bn': 256}),
    'f16s_256x9_cin96_d2': (96, 256, 9, 2, False, False, 'f16s', {}),
    'f16s_128x9_cin32_d4_res': (32, 128, 9, 4, True, True, 'f16s', {}),
    'f16s_128x1_cin32': (32, 128, 1, 1, False, False, 'f16s', {}),
    'f16s_256x1_cin160_res': (160, 256, 1, 1, True, False, 'f16s', {}),
    'p16_64_cin64_res': (64, 64, 9, 1, True, True, 'f16s', {}),                    # k_conv3x3_p16
    'p16_64_cin96_d2': (96, 64, 9, 2, False, True, 'f16s', {}),
    'p16_128_cin96_d3': (96, 128, 9, 3, False, False, 'f16s', {}),
    'p16_128_cin64_d1_res': (64, 128, 9, 1, True, True, 'f16s', {}),
    'pred_64_cin64_d2_res': (64, 64, 9, 2, True, True, 'pred', {}),                # the predecessor of k_conv3x3_p16
    'pred_128_cin96_d4': (96, 128, 9, 4, False, True, 'pred', {}),
}


def _flat_1x1(n_cu, B, H, W, **kw):
    """spa_conv1x1_f16s as Engine.conv3x3_f16s calls it: every image one row of H x W pixels"""
    return conv_f32(n_cu, B, 1, H * W, **kw)


def plan_direct(name, target, n_cu):
    Cin, Cout, taps, dil, res, relu, path, want = DIRECT[name]
    split = path != 'f32'
    fn = _flat_1x1 if (split and taps == 1) else conv_f32
    key = form('direct:' + name, fn, Cin=Cin, Cout=Cout, taps=taps, split=split, convp=path != 'pred')
    return pick(target, key, n_cu, dil=dil, bns=(128, 256, 512) if split else (128, 256), want=tuple(want.items()))


# name: (Cin, Cout, csplit, split): csplit < Cout = the 1x1 stride-2 projection as the channels csplit..
STRIDE2 = {
    's2_f16s_128_proj': (32, 128, 64, True),
    's2_f16s_256_cin96': (96, 256, 256, True),
    's2_f32_256_proj': (64, 256, 128, False),
    's2_f32_128_cin32': (32, 128, 128, False),
}


def plan_stride2(name, target, n_cu):
    Cin, Cout, csplit, split = STRIDE2[name]
    return pick(target, form('s2:' + name, conv_s2, Cin=Cin, Cout=Cout, split=split), n_cu, bns=(256,), Hi_min=7)


# name: (Cin, Cout, dil, res, relu, tile, split)
WINO = {
    'w16_256_cin64_res': (64, 256, 1, True, True, 4, True),        # k_gemm_f16x3_stag<256,256>
    'w16_256_cin32_d2': (32, 256, 2, False, True, 4, True),        # nk 1
    'w16_512_cin160_d3': (160, 512, 3, True, False, 4, True),      # nk 5, two channel tiles
    'w16_128_cin32_d1': (32, 128, 1, False, False, 4, True),       # k_gemm_f16x3<128,128>, nk 1
    'w16_384_cin96_d4_res': (96, 384, 4, True, True, 4, True),     # nk 3, three channel tiles
    'w32_f4_256_cin32': (32, 256, 1, False, True, 4, False),       # k_conv3x3_f32<256,1,256>, 36 problems, nk 1
    'w32_f2_128_cin96_res': (96, 128, 2, True, True, 2, False),    # 16 problems, nk 3
}


def plan_wino(name, target, n_cu, L):
    """L: the library (its spa_wino4_tiles / spa_wino_tiles)"""
    Cin, Cout, dil, _, _, tile, split = WINO[name]
    rows_fn = L.spa_wino4_tiles if tile == 4 else L.spa_wino_tiles
    if split:
        return pick_wino(target, n_cu, rows_fn, Cin, Cout, dil)
    return pick_wino(target, n_cu, rows_fn, Cin, Cout, dil, gemm=conv_f32, zcount=36 if tile == 4 else 16)


# name: (Cin, Cout, stride, proj, res, relu)
SMALL = {
    'small_16_16_res': (16, 16, 1, False, True, True),
    'small_16_32_s2_proj': (16, 32, 2, True, False, True),
    'small_32_32_res': (32, 32, 1, False, True, True),
}


def plan_small(name, target, n_cu):
    stride = SMALL[name][2]
    return pick(target, form('small:' + name, conv_small, stride=stride), n_cu, bns=(32 * stride,), Hi_min=3 if stride == 1 else 5)


def plan_layer2(target, n_cu):
    return pick(target, form('layer2', drn_layer2), n_cu, bns=(64,), Hi_min=5)


# name: (Cin, Cout, taps, stride, dil, res, relu)
LIGHT = {
    'light_3x3_s1_64_128_d2_res': (64, 128, 9, 1, 2, True, True),
    'light_3x3_s2_32_128': (32, 128, 9, 2, 1, False, True),
    'light_1x1_s1_128_256': (128, 256, 1, 1, 1, False, False),
}


def plan_light(name, target, n_cu):
    Cin, Cout, taps, stride, dil, res, relu = LIGHT[name]
    key = form('light:' + name, conv_bf16_light, Cin=Cin, Cout=Cout, taps=taps, stride=stride)
    return pick(target, key, n_cu, dil=dil, bns=(64 * stride,), want=(('full', True),))
