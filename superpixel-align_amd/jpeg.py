"""The demo movie's JPEG frames whose entropy-coded scan is made on the device (--jpeg_encoder device).

Engine.jpeg_encode (spa_jpeg_encode_rgb8, csrc/spa_jpeg.hip) leaves one scan per frame: the entropy-coded bytes of a
baseline sequential JFIF, 8-bit, YCbCr 4:2:0, Pillow's quality-75 tables, cut into restart intervals of Ri MCUs.
`assemble` adds what makes that a file, on the host: SOI, Pillow's APP0, the two DQT, SOF0, the four DHT, DRI, SOS,
then the scan and EOI.  The bytes are this project's, not libjpeg's (another colour conversion, another DCT, restart
markers); they are fixed in include/spalign.h so that the device and `encode_host` can be compared byte for byte.

encode_host is the plain numpy / Python restatement of that format, written for the tests; it is never on a product
path.  The tables below are data: the quality-75 quantisation tables and the standard Huffman tables as Pillow writes
them (tests/test_jpeg_device_cpu.py reads them back out of a file Pillow writes).  DeviceEncoder is what the batch
loops use: devenc.Ring, the buffer ring of every device encoder, with this module's bound, engine call and framing.
"""
import struct

import numpy as np

from . import devenc

MCU = 16                                                 # pixels per side of a 4:2:0 minimum coded unit
DEFAULT_RI = 4                                           # restart interval in MCUs (README "JPEG frames on the device": why 4)

# zigzag position k -> natural index 8 * v + u
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
          60, 61, 54, 47, 55, 62, 63)

# quantisation tables at quality 75, in zigzag order (as a DQT segment holds them)
Q_LUMA = (8, 6, 6, 7, 6, 5, 8, 7, 7, 7, 9, 9, 8, 10, 12, 20, 13, 12, 11, 11, 12, 25, 18, 19, 15, 20, 29, 26, 31, 30,
          29, 26, 28, 28, 32, 36, 46, 39, 32, 34, 44, 35, 28, 28, 40, 55, 41, 44, 48, 49, 52, 52, 52, 31, 39, 57, 61,
          56, 50, 60, 46, 51, 52, 50)
Q_CHROMA = (9, 9, 9, 12, 11, 12, 24, 13, 13, 24, 50, 33, 28, 33) + (50,) * 50

# Huffman tables: (the number of codes of each length 1..16, the symbols in code order)
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), tuple(bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738'
    '393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5'
    'a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), tuple(bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637'
    '38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3'
    'a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')))

# the DCT matrix: T[u][x] = round(8192 * 1/2 * c(u) * cos((2x + 1) u pi / 16)), c(0) = 1 / sqrt(2)
DCT = ((2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896),
       (4017, 3406, 2276, 799, -799, -2276, -3406, -4017),
       (3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784),
       (3406, -799, -4017, -2276, 2276, 4017, 799, -3406),
       (2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896),
       (2276, -4017, 799, 3406, -3406, -799, 4017, -2276),
       (1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567),
       (799, -2276, 3406, -4017, 4017, -3406, 2276, -799))

# what a block can take at most: the longest DC code (11 bits, chrominance) and the 11 bits of the largest baseline
# DC category, then 63 coefficients of a 16-bit code and 10 bits each
BLOCK_BITS_MAX = (11 + 11) + 63 * (16 + 10)
MCU_BYTES_MAX = 6 * BLOCK_BITS_MAX // 8                  # 1245; 6 * 1660 is a multiple of 8


def check_shape(H, W, Ri):
    H, W, Ri = int(H), int(W), int(Ri)
    if H <= 0 or W <= 0 or H % MCU or W % MCU:
        raise ValueError('jpeg: a frame must be a multiple of 16 in both directions, got %d x %d' % (H, W))
    if Ri < 1 or Ri > 65535:
        raise ValueError('jpeg: the restart interval must be 1..65535 MCUs, got %d' % Ri)
    return H, W, Ri


def scan_bound(H, W, Ri):
    """spa_jpeg_scan_bound: bytes that hold the scan of any (H, W) frame.  An MCU is at most MCU_BYTES_MAX bytes of
    codes, an interval's padding completes a byte that the count already holds, every byte may be 0xFF and stuffed, and
    every interval but the last ends in a 2-byte marker.  0 for arguments the encoder refuses."""
    H, W, Ri = int(H), int(W), int(Ri)
    if H <= 0 or W <= 0 or H % MCU or W % MCU or Ri < 1:
        return 0
    n_mcu = (H // MCU) * (W // MCU)
    n_int = (n_mcu + Ri - 1) // Ri
    return 2 * MCU_BYTES_MAX * n_mcu + 2 * (n_int - 1)


def huffman_codes(table):
    """{symbol: (code, length)} of a (counts, symbols) table: canonical codes, JPEG Annex C"""
    counts, symbols = table
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def ycc420(rgb):
    """(H,W,3) uint8 -> (Y (H,W), Cb (H/2,W/2), Cr (H/2,W/2)) int32 samples 0..255"""
    p = np.asarray(rgb).astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + 8421375) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + 8421375) >> 16

    def sub(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    return Y, sub(Cb), sub(Cr)


def quantised_blocks(plane, q_zigzag):
    """(h,w) samples -> (h/8, w/8, 64) int64: every 8x8 block's quantised coefficients in zigzag order"""
    h, w = plane.shape
    s = (plane.astype(np.int64) - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)       # (by, bx, y, x)
    T = np.array(DCT, dtype=np.int64)
    a = (np.einsum('ux,ijyx->ijyu', T, s) + 1024) >> 11
    b = np.einsum('vy,ijyu->ijvu', T, a)
    assert np.abs(b).max() < (1 << 31)
    Q = np.empty(64, dtype=np.int64)
    Q[list(ZIGZAG)] = q_zigzag
    d = Q.reshape(8, 8) << 15
    q = np.sign(b) * ((np.abs(b) + d // 2) // d)
    return q.reshape(h // 8, w // 8, 64)[:, :, list(ZIGZAG)]


def mcu_coefficients(rgb):
    """(H,W,3) uint8 -> (nMCU, 6, 64) int64: per MCU in raster order the blocks Y00 Y01 Y10 Y11 Cb Cr, zigzag order:
    what the transform kernel leaves in coef_ws"""
    H, W = np.asarray(rgb).shape[:2]
    Y, Cb, Cr = ycc420(rgb)
    yq, bq, rq = quantised_blocks(Y, Q_LUMA), quantised_blocks(Cb, Q_CHROMA), quantised_blocks(Cr, Q_CHROMA)
    my, mx = H // MCU, W // MCU
    out = np.empty((my, mx, 6, 64), dtype=np.int64)
    out[:, :, 0], out[:, :, 1] = yq[0::2, 0::2], yq[0::2, 1::2]
    out[:, :, 2], out[:, :, 3] = yq[1::2, 0::2], yq[1::2, 1::2]
    out[:, :, 4], out[:, :, 5] = bq, rq
    return out.reshape(my * mx, 6, 64)


def category(v):
    return int(abs(int(v))).bit_length()


class _Interval(object):
    """one restart interval's bytes: bits most-significant first, a 0x00 after every 0xFF"""

    def __init__(self, counters):
        self.acc, self.n, self.out, self.c = 0, 0, bytearray(), counters

    def put(self, value, nbits):
        self.acc = (self.acc << nbits) | value
        self.n += nbits
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.n -= 8
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
                self.c['stuffed'] += 1
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            before = self.c['stuffed']
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
            self.c['stuffed_pad'] += self.c['stuffed'] - before
        return bytes(self.out)


COUNTERS = ('zrl', 'no_eob', 'stuffed', 'stuffed_pad', 'dc_pos_cat', 'dc_neg_cat', 'ac_cat', 'intervals')


def _block(bits, coef, pred, dc, ac, c):
    diff = int(coef[0]) - pred
    cat = category(diff)
    bits.put(*dc[cat])
    if cat:
        bits.put(diff if diff > 0 else diff - 1 + (1 << cat), cat)
        key = 'dc_pos_cat' if diff > 0 else 'dc_neg_cat'
        c[key] = max(c[key], cat)
    run = 0
    for k in range(1, 64):
        v = int(coef[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])
            c['zrl'] += 1
            run -= 16
        cat = category(v)
        c['ac_cat'] = max(c['ac_cat'], cat)
        bits.put(*ac[(run << 4) | cat])
        bits.put(v if v > 0 else v - 1 + (1 << cat), cat)
        run = 0
    if run:
        bits.put(*ac[0x00])
    else:
        c['no_eob'] += 1
    return int(coef[0])


def encode_intervals(rgb, Ri):
    """-> (the list of every restart interval's stuffed bytes, without markers; the counters)"""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError('jpeg.encode_host: an (H, W, 3) uint8 frame, got %s %s' % (rgb.shape, rgb.dtype))
    H, W, Ri = check_shape(rgb.shape[0], rgb.shape[1], Ri)
    coef = mcu_coefficients(rgb)
    tabs = [(huffman_codes(DC_LUMA), huffman_codes(AC_LUMA))] * 4 + [(huffman_codes(DC_CHROMA), huffman_codes(AC_CHROMA))] * 2
    c = dict.fromkeys(COUNTERS, 0)
    intervals = []
    for lo in range(0, len(coef), Ri):
        bits, pred = _Interval(c), [0, 0, 0]
        for m in range(lo, min(lo + Ri, len(coef))):
            for j in range(6):
                comp = max(j - 3, 0)
                pred[comp] = _block(bits, coef[m, j], pred[comp], tabs[j][0], tabs[j][1], c)
        intervals.append(bits.finish())
    c['intervals'] = len(intervals)
    return intervals, c


def join_intervals(intervals):
    return b''.join(iv + (bytes((0xFF, 0xD0 + (k & 7))) if k + 1 < len(intervals) else b'')
                    for k, iv in enumerate(intervals))


def encode_host(rgb, Ri=DEFAULT_RI, counters=None):
    """(H,W,3) uint8 -> the scan spa_jpeg_encode_rgb8 writes for that frame: the intervals' bytes, FF D0+(k mod 8)
    after every interval but the last.  counters: a dict that receives COUNTERS."""
    intervals, c = encode_intervals(rgb, Ri)
    if counters is not None:
        counters.update(c)
    return join_intervals(intervals)


def _segment(marker, body):
    return bytes((0xFF, marker)) + struct.pack('>H', len(body) + 2) + body


def _dht(tc_th, table):
    return _segment(0xC4, bytes((tc_th,)) + bytes(table[0]) + bytes(table[1]))


def header(H, W, Ri):
    """everything before the scan"""
    H, W, Ri = check_shape(H, W, Ri)
    if H > 65535 or W > 65535:
        raise ValueError('jpeg.assemble: %d x %d does not fit SOF0\'s 16-bit fields' % (H, W))
    return (b'\xff\xd8' + _segment(0xE0, b'JFIF\0' + bytes((1, 1, 0, 0, 1, 0, 1, 0, 0))) +
            _segment(0xDB, b'\x00' + bytes(Q_LUMA)) + _segment(0xDB, b'\x01' + bytes(Q_CHROMA)) +
            _segment(0xC0, struct.pack('>BHHB', 8, H, W, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1))) +
            _dht(0x00, DC_LUMA) + _dht(0x10, AC_LUMA) + _dht(0x01, DC_CHROMA) + _dht(0x11, AC_CHROMA) +
            _segment(0xDD, struct.pack('>H', Ri)) +
            _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))))


def assemble(scan_bytes, H, W, Ri):
    """the JPEG file of an (H, W) frame from its scan"""
    return header(H, W, Ri) + bytes(scan_bytes) + b'\xff\xd9'


class DeviceEncoder(devenc.Ring):
    """devenc.Ring for JPEG frames from device images: encode(frames) leaves the scans of frames (n,H,W,3) uint8 with
    their lengths (each set has its own coefficient workspace), file_bytes(slot, j) is frame j's JPEG file.
    pinned_bytes: the ring's first pinned buffer; by default a byte per pixel, far above what quality 75 takes."""

    def __init__(self, engine, shape, batch, Ri=DEFAULT_RI, pinned_bytes=None):
        import torch
        H, W, self.Ri = check_shape(shape[0], shape[1], Ri)
        self.shape = (H, W)
        bound = scan_bound(H, W, self.Ri)
        if bound > (1 << 31) - 1:
            raise ValueError('jpeg.DeviceEncoder: the scan of a %d x %d frame may not fit 2^31 - 1 bytes' % self.shape)
        B = max(int(batch), 1)
        if pinned_bytes is None:
            pinned_bytes = min(B * H * W, B * ((bound + 15) // 16 * 16))
        devenc.Ring.__init__(self, engine, B, bound, 1, pinned_bytes)
        self.declare('coef', (B * (H // MCU) * (W // MCU) * 384,), torch.int16)

    def launch(self, slot, frames, n):
        self.eng.jpeg_encode(frames, self.Ri, out=slot['out'][:n], nbytes=slot['meta'][0, :n], coef=slot['coef'])

    def frame(self, slot, j, payload):
        return assemble(payload, self.shape[0], self.shape[1], self.Ri)


