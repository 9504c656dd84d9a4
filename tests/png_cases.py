"""The images of the label-PNG encoder's tests (test_png_device_cpu.py, test_gpu_png_device.py) and the check that a
file made from a stream is a PNG of the image: the smallest shapes that reach each branch of the format fixed in
include/spalign.h (spa_png_deflate_u8).

  noise 1x1, 1x2, 5x3, 17x67          8- and 9-bit literals, no runs
  all-0 / all-255, 3 rows, widths     2, 3, 4 (a run too short for a match / of exactly one match), 257..262, 516..520
                                      and 775: remainders 0, 1 and 2 after one, two and three full matches of 258 (the
                                      scanline is the width + 1 bytes; in row 0 of the all-255 image the run value is a
                                      9-bit literal)
  wedge 64x700                        a road-like mask
  B = 3, the middle image noise       offsets across images
  B = 3 of 700x33                     2 100 rows: more than one workgroup's, and more than one row per scan thread
  2x5000                              runs of thousands
  96x192 -> 192x384, 37x53 -> 64x100  the nearest-neighbour tables
  B = 2 of 40x128 speckle, 9x48 noise widths that are multiples of 16: the kernel's 16-byte loads (every width above takes
                                      its byte loads)
"""
import io
import struct
import zlib

import numpy as np

FLAT_WIDTHS = [2, 3, 4] + list(range(257, 263)) + list(range(516, 521)) + [775]
NEAREST = [((96, 192), (192, 384)), ((37, 53), (64, 100))]


def wedge(H=64, W=700):
    yy, xx = np.mgrid[0:H, 0:W]
    return (np.abs(xx - W // 2) < 4 * yy).astype(np.uint8)


def cases():
    """[(name, src (B,Hs,Ws) uint8, out_shape or None)], the same arrays in every call"""
    rng = np.random.RandomState(20260)
    out = []
    for shape in [(1, 1), (1, 2), (5, 3), (17, 67)]:
        out.append(('noise_%dx%d' % shape, rng.randint(0, 256, (1,) + shape).astype(np.uint8), None))
    for w in FLAT_WIDTHS:
        for v in (0, 255):
            out.append(('flat%d_w%d' % (v, w), np.full((1, 3, w), v, np.uint8), None))
    out.append(('wedge_64x700', wedge()[None], None))
    out.append(('batch3_noise_in_the_middle', np.stack([wedge(), rng.randint(0, 256, (64, 700)).astype(np.uint8),
                                                        1 - wedge()]), None))
    out.append(('batch3_700x33', (rng.rand(3, 700, 33) < 0.3).astype(np.uint8), None))
    long_rows = np.zeros((1, 2, 5000), np.uint8)
    long_rows[0, 0, 100:4000] = 1
    long_rows[0, 1, 7:] = 200
    out.append(('long_2x5000', long_rows, None))
    speckle = np.repeat(wedge(40, 128)[None], 2, 0)
    speckle[rng.rand(2, 40, 128) < 0.01] ^= 1
    out.append(('speckle_40x128', speckle, None))
    out.append(('noise_9x48', rng.randint(0, 256, (1, 9, 48)).astype(np.uint8), None))
    for src, dst in NEAREST:
        out.append(('nearest_%dx%d_to_%dx%d' % (src + dst), (rng.rand(2, *src) < 0.4).astype(np.uint8) * 7, dst))
    return out


# ------------------------------------------------------------------------------- a strict RFC 1951 reader
# zlib's inflate is lenient where the RFC is not (it takes length code 284 with 31 extra as 258), so the check below also
# reads the stream with this reader: one block, BFINAL = 1, BTYPE = 01, the fixed codes, every length code inside its
# range, symbol 256, zero padding, nothing after it.
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
              6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


class StreamError(ValueError):
    pass


def strict_inflate_fixed(stream):
    bits = ''.join(format(b, '08b')[::-1] for b in stream)         # the order deflate reads them in
    pos = [0]

    def take(n):
        if pos[0] + n > len(bits):
            raise StreamError('the stream ends inside a token')
        s = bits[pos[0]:pos[0] + n]
        pos[0] += n
        return s

    def field(n):                                                  # least-significant bit first
        return int(take(n)[::-1], 2) if n else 0

    def code(n):                                                   # most-significant bit first
        return int(take(n), 2)

    if field(1) != 1 or field(2) != 1:
        raise StreamError('not one final fixed-Huffman block')
    out = bytearray()
    while True:
        c = code(7)
        if c <= 0x17:
            sym = 256 + c
        else:
            c = (c << 1) | code(1)
            if 0x30 <= c <= 0xBF:
                sym = c - 0x30
            elif 0xC0 <= c <= 0xC7:
                sym = 280 + c - 0xC0
            else:
                sym = 144 + ((c << 1) | code(1)) - 0x190
        if sym < 256:
            out.append(sym)
            continue
        if sym == 256:
            break
        if sym > 285:
            raise StreamError('length symbol %d' % sym)
        extra = field(_LEN_EXTRA[sym - 257])
        length = _LEN_BASE[sym - 257] + extra
        if sym == 284 and extra == 31:
            raise StreamError('length 258 written as code 284 + 31: outside the code\'s range 227..257')
        d = code(5)
        if d > 29:
            raise StreamError('distance code %d' % d)
        dist = _DIST_BASE[d] + field(_DIST_EXTRA[d])
        if dist > len(out):
            raise StreamError('distance %d before the start' % dist)
        for _ in range(length):
            out.append(out[-dist])
    if '1' in bits[pos[0]:] or len(bits) - pos[0] >= 8:
        raise StreamError('bits after the end of the block')
    return bytes(out)


def chunks(data):
    """[(tag, body)] of a PNG file; the signature and every CRC are checked"""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    out, p = [], 8
    while p < len(data):
        n, = struct.unpack('>I', data[p:p + 4])
        tag, body = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        assert struct.unpack('>I', data[p + 8 + n:p + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        out.append((tag, body))
        p += 12 + n
    assert p == len(data)
    return out


def check_file(png, data, img):
    """data is `img` as an 8-bit greyscale PNG made of one Up-filtered fixed-Huffman stream: raises otherwise
    (AssertionError, zlib.error, StreamError, or what Pillow raises)"""
    from PIL import Image
    H, W = img.shape
    parts = chunks(data)
    assert [t for t, _ in parts] == [b'IHDR', b'IDAT', b'IEND']
    assert parts[0][1] == struct.pack('>IIBBBBB', W, H, 8, 0, 0, 0, 0) and parts[2][1] == b''
    body = parts[1][1]
    assert body[:2] == b'\x78\x01' and len(body) - 6 <= png.deflate_bound(H, W)
    rows = png.filtered_scanlines(img).tobytes()
    assert zlib.decompress(body) == rows                           # zlib checks the Adler-32 itself
    assert strict_inflate_fixed(body[2:-4]) == rows
    with Image.open(io.BytesIO(data)) as f:
        assert f.mode == 'L' and f.size == (W, H)
        assert np.array_equal(np.asarray(f), img)
