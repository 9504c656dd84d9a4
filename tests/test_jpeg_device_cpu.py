"""The host side of --jpeg_encoder device, without a GPU: jpeg.encode_host (the restatement of the scan that
spa_jpeg_encode_rgb8 writes) and jpeg.assemble on the frames of jpeg_cases.py, at the restart intervals 1, 3, one MCU
row and one interval for the whole frame.  Pillow must open every file with warnings as errors; its quality must be
Pillow's own; its size must be Pillow's but for what restart intervals cost; intervals must not depend on each other;
and the cases together must reach every branch of the entropy coder.  MjpegAviWriter.write_encoded is checked here
too."""
import importlib
import math
import os

import numpy as np
import pytest

import jpeg_cases as jc
from test_demovideo_cpu import parse_avi

jpeg = importlib.import_module('superpixel-align_amd.jpeg')
dv = importlib.import_module('superpixel-align_amd.demovideo')
CASES = jc.cases()
IDS = [c[0] for c in CASES]
PSNR_MARGIN_DB = 0.3                         # twice the worst shortfall of the prototype that the format was fixed with
RI1_BYTES_PER_MCU = 4                        # see test_file_size_is_pillows_but_for_the_intervals


@pytest.fixture(scope='module')
def encoded():
    """{(name, Ri): (scan, counters)}, computed once"""
    memo = {}
    for name, frame in CASES:
        for Ri in jc.intervals_for(frame):
            c = {}
            memo[name, Ri] = (jpeg.encode_host(frame, Ri, c), c)
    return memo


def test_tables_and_segments_are_the_ones_pillow_writes():
    frame = jc.noise(3, (32, 48))
    segs, _ = jc.segments(jc.pillow_jpeg(frame))
    dqt = [body for m, body in segs if m == 0xDB]
    dht = {body[0]: body[1:] for m, body in segs if m == 0xC4}
    assert dqt == [b'\x00' + bytes(jpeg.Q_LUMA), b'\x01' + bytes(jpeg.Q_CHROMA)]
    assert sorted(dht) == [0x00, 0x01, 0x10, 0x11]
    for key, table in ((0x00, jpeg.DC_LUMA), (0x10, jpeg.AC_LUMA), (0x01, jpeg.DC_CHROMA), (0x11, jpeg.AC_CHROMA)):
        assert dht[key] == bytes(table[0]) + bytes(table[1]), hex(key)
        assert sum(table[0]) == len(table[1])
    # our header: Pillow's segments in Pillow's order, then DRI, then Pillow's SOS
    ours, at = jc.segments(jpeg.assemble(b'', 32, 48, 7))
    assert [s for s in ours if s[0] != 0xDD] == segs
    assert [m for m, _ in ours] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert dict(ours)[0xDD] == b'\x00\x07'
    assert dict(ours)[0xC0] == bytes((8, 0, 32, 0, 48, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1))
    assert dict(ours)[0xDA] == bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))
    assert jpeg.assemble(b'', 32, 48, 7)[at:] == b'\xff\xd9'
    # the DCT matrix, from its definition
    T = [[int(round(8192 * 0.5 * (math.sqrt(0.5) if u == 0 else 1.0) * math.cos((2 * x + 1) * u * math.pi / 16)))
          for x in range(8)] for u in range(8)]
    assert tuple(tuple(r) for r in T) == jpeg.DCT
    assert sorted(jpeg.ZIGZAG) == list(range(64)) and jpeg.ZIGZAG[:6] == (0, 1, 8, 16, 9, 2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                               'spalign.h')).read()
    flat = ''.join(header.split())
    assert ''.join(('{' + ','.join('{' + ','.join(str(v) for v in r) + '}' for r in T) + '}').split()) in \
        flat.replace('\\', '')


def test_scan_bound_is_the_librarys_and_above_every_scan(encoded):
    lib = importlib.import_module('superpixel-align_amd._lib').lib()
    for H, W, Ri in [(16, 16, 1), (16, 32, 5), (64, 96, 3), (1024, 2048, 1), (1024, 2048, 8), (1024, 2048, 1 << 20),
                     (24, 32, 1), (32, 40, 1), (0, 16, 1), (16, 16, 0), (-16, 16, 1)]:
        assert int(lib.spa_jpeg_scan_bound(H, W, Ri)) == jpeg.scan_bound(H, W, Ri), (H, W, Ri)
    assert jpeg.scan_bound(16, 16, 1) == 2 * 1245 and jpeg.scan_bound(24, 32, 1) == 0
    assert jpeg.scan_bound(32, 32, 3) == 4 * 2 * 1245 + 2
    assert jpeg.BLOCK_BITS_MAX == 1660 and 6 * jpeg.BLOCK_BITS_MAX == 8 * jpeg.MCU_BYTES_MAX
    # no code is longer than the bound assumes
    for dc, ac in ((jpeg.DC_LUMA, jpeg.AC_LUMA), (jpeg.DC_CHROMA, jpeg.AC_CHROMA)):
        assert max(n for _, n in jpeg.huffman_codes(dc).values()) <= 11 and max(dc[1]) <= 11
        assert max(n for _, n in jpeg.huffman_codes(ac).values()) <= 16 and max(s & 15 for s in ac[1]) <= 10
    for name, frame in CASES:
        for Ri in jc.intervals_for(frame):
            assert len(encoded[name, Ri][0]) < jpeg.scan_bound(frame.shape[0], frame.shape[1], Ri)
    for bad in ((24, 32, 1), (16, 16, 0), (16, 16, 65536)):
        with pytest.raises(ValueError):
            jpeg.check_shape(*bad)
    with pytest.raises(ValueError):
        jpeg.encode_host(np.zeros((16, 16, 3), np.float32), 1)
    with pytest.raises(ValueError):
        jpeg.encode_host(np.zeros((16, 24, 3), np.uint8), 1)


@pytest.mark.parametrize('name,frame', CASES, ids=IDS)
def test_pillow_decodes_the_file_at_pillows_quality(encoded, name, frame):
    """The restatement's PSNR against the source is at least Pillow's own quality-75 PSNR minus 0.3 dB.  Measured
    shortfalls (Pillow's PSNR minus ours, the same at every Ri): edge 0.000, chroma 0.009, checker 0.000, noise 0.003,
    smooth -0.261 (ours is better); mcus is lossless in both and counts as equal."""
    H, W = frame.shape[:2]
    want = jc.psnr(frame, jc.decode(jc.pillow_jpeg(frame)))
    for Ri in jc.intervals_for(frame):
        got = jc.decode(jpeg.assemble(encoded[name, Ri][0], H, W, Ri))
        assert got.shape == (H, W, 3)
        ours = jc.psnr(frame, got)
        print('%s Ri %d: PSNR %.3f dB, Pillow %.3f dB' % (name, Ri, ours, want))
        assert (ours == want) if math.isinf(want) else (ours >= want - PSNR_MARGIN_DB), (Ri, ours, want)


@pytest.mark.parametrize('name,frame', CASES, ids=IDS)
def test_file_size_is_pillows_but_for_the_intervals(encoded, name, frame):
    """One interval: no larger than Pillow's file plus 16 bytes, of which the DRI segment is 6.  Ri = 1: measured
    against Pillow's files, these cases cost 1.5 (chroma) to 2.83 (mcus) bytes per MCU beyond the DRI segment -- the
    2-byte marker, the padding, and DC values coded from 0 instead of as differences; the bound is 4 per MCU, a byte
    above the worst."""
    H, W = frame.shape[:2]
    n_mcu = (H // 16) * (W // 16)
    pillow = len(jc.pillow_jpeg(frame))
    whole = len(jpeg.assemble(encoded[name, n_mcu + 5][0], H, W, n_mcu + 5))
    each = len(jpeg.assemble(encoded[name, 1][0], H, W, 1))
    print('%s: Pillow %d, one interval %d, Ri = 1 %d (%.2f per MCU)' % (name, pillow, whole, each,
                                                                         (each - pillow - 6) / n_mcu))
    assert whole <= pillow + 16
    assert each <= pillow + 16 + RI1_BYTES_PER_MCU * n_mcu


def test_intervals_do_not_depend_on_each_other():
    frame = jc.noise(7, (32, 48))                        # 6 MCUs, 3 per row
    other = frame.copy()
    other[16:32, 16:32] = 255 - other[16:32, 16:32]      # MCU 4
    for Ri in (1, 2, 3):
        a, _ = jpeg.encode_intervals(frame, Ri)
        b, _ = jpeg.encode_intervals(other, Ri)
        assert len(a) == len(b) == -(-6 // Ri)
        for k in range(len(a)):
            assert (a[k] != b[k]) == (k == 4 // Ri), (Ri, k)
        # the scan: the intervals in order, a marker behind every one but the last
        scan = jpeg.encode_host(frame, Ri)
        want = b''.join(iv + (bytes((0xFF, 0xD0 + k % 8)) if k + 1 < len(a) else b'') for k, iv in enumerate(a))
        assert scan == want


def test_the_cases_reach_every_branch_of_the_entropy_coder(encoded):
    most = dict.fromkeys(jpeg.COUNTERS, 0)
    for c in (v[1] for v in encoded.values()):
        assert sorted(c) == sorted(jpeg.COUNTERS)
        for k in most:
            most[k] = max(most[k], c[k])
    assert most['zrl'] > 0 and most['no_eob'] > 0 and most['stuffed'] > 0 and most['stuffed_pad'] > 0, most
    assert most['intervals'] > 8, most
    # the largest categories: |DC| <= 128 for Y at Q = 8, so a difference is at most 255: category 8.  An AC
    # coefficient is largest at (0,1): 128 * 23168 * 20996 / 2^26 = 928 over Q = 6, 154: category 8
    assert most['dc_pos_cat'] == 8 and most['dc_neg_cat'] == 8 and most['ac_cat'] == 8, most
    T = np.abs(np.array(jpeg.DCT, dtype=np.int64)).sum(axis=1)
    Q = np.empty(64, np.int64)
    Q[list(jpeg.ZIGZAG)] = jpeg.Q_LUMA
    reach = (128 * T[:, None] * T[None, :] / 2.0 ** 26) / Q.reshape(8, 8)
    reach[0, 0] = 0
    assert 128 <= reach.max() < 255


def test_both_flags_default_to_pillow_and_sizes_are_checked():
    parse = dv.demovideo_parser().parse_args
    assert parse([]).jpeg_encoder == 'pillow' and parse(['--jpeg_encoder', 'device']).jpeg_encoder == 'device'
    with pytest.raises(SystemExit):
        parse(['--jpeg_encoder', 'turbo'])
    # refused by the parser, before a device or a snapshot is touched
    with pytest.raises(SystemExit):
        dv.demovideo_main(['--jpeg_encoder', 'device', '--out_video_fn', 'x.avi', '--eval_shape', '1000', '2048'])


def test_write_encoded_keeps_call_order(tmp_path):
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in range(5)]
    ours = [jpeg.assemble(jpeg.encode_host(f, 2), 48, 64, 2) for f in frames]
    fn = str(tmp_path / 'm.avi')
    w = dv.MjpegAviWriter(fn, (64, 48), encode_threads=3)
    order = 'wewweewe'                                   # w: write(), e: write_encoded()
    want = []
    for k, op in enumerate(order):
        if op == 'w':
            w.write(frames[k % 5])
            want.append(dv.encode_jpeg(frames[k % 5]))
        else:
            w.write_encoded(ours[k % 5])
            want.append(ours[k % 5])
    for bad in (b'', b'\xff\xd8', ours[0][:-2], ours[0][2:], frames[0], None):
        with pytest.raises(ValueError, match='write_encoded'):
            w.write_encoded(bad)
    w.close()
    with pytest.raises(ValueError, match='closed'):
        w.write_encoded(ours[0])
    a = parse_avi(open(fn, 'rb').read())
    assert a['frames'] == want and a['avih'][4] == len(order)
    for k in range(len(order)):
        assert a['index'][k][3] == len(want[k]) and a['movi'] + a['index'][k][2] == a['chunk_at'][k]
        assert jc.decode(a['frames'][k]).shape == (48, 64, 3)
