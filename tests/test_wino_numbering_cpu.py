"""The interleaved numbering of the Winograd tiles (csrc/spa_wino_dev.h: wino_tile) on the host: for every map of
tests/test_gpu_wino_operands.py and every dilation of the network it must enumerate exactly the (image, sub-grid, tile row,
tile column) set the sub-grid-major numbering did — a bijection on [0, T) — start consecutive ids of a row at consecutive
pixel columns, and be the old numbering itself at dilation 1.  No GPU: the decode is plain C++ (spa_wino4_tile_decode)."""
import ctypes

import pytest

# (B, H, W) of the GPU test's maps x the network's dilations
MAPS = [(2, 22, 38), (2, 9, 7), (3, 36, 52), (1, 16, 24)]


def _decode(L, B, H, W, d, interleaved):
    out = (ctypes.c_int32 * 5)()
    T = B * d * d * ((-(-H // d) + 3) // 4) * ((-(-W // d) + 3) // 4)
    assert int(L.spa_wino4_tiles(B, H, W, d)) == (T + 255) // 256 * 256
    tiles = []
    for t in range(T):
        assert L.spa_wino4_tile_decode(B, H, W, d, interleaved, t, out) == 0
        tiles.append(tuple(out))
    assert L.spa_wino4_tile_decode(B, H, W, d, interleaved, T, out) != 0          # T itself is outside
    return tiles


@pytest.mark.parametrize('d', [1, 2, 4])
@pytest.mark.parametrize('B,H,W', MAPS)
def test_interleaved_numbering_is_a_bijection_onto_the_old_set(spa, B, H, W, d):
    L = spa._lib.lib()
    old, new = _decode(L, B, H, W, d, 0), _decode(L, B, H, W, d, 1)
    th, tw = (-(-H // d) + 3) // 4, (-(-W // d) + 3) // 4
    want = {(b, sy, sx, ty, tx) for b in range(B) for sy in range(d) for sx in range(d) for ty in range(th) for tx in range(tw)}
    assert len(old) == len(want) and set(old) == want
    assert len(set(new)) == len(new) and set(new) == want
    if d == 1:
        assert new == old
    # the formula: t = ((b * d + sy) * th + ty) * tw * d + gx with gx = tx * d + sx
    for t, (b, sy, sx, ty, tx) in enumerate(new):
        assert t == ((b * d + sy) * th + ty) * tw * d + tx * d + sx
    # consecutive ids inside a row: the first pixel column of the tile moves on by ONE pixel inside a group of d, and to the
    # next group of 4 d columns after it
    for t in range(1, len(new)):
        (b0, sy0, sx0, ty0, tx0), (b1, sy1, sx1, ty1, tx1) = new[t - 1], new[t]
        if t % (tw * d):
            assert (b1, sy1, ty1) == (b0, sy0, ty0)
            assert (sx1 + 4 * tx1 * d) - (sx0 + 4 * tx0 * d) == (1 if sx1 else 3 * d + 1)
