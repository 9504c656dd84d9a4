"""Label PNGs whose compressed payload is made on the device (--png_encoder device).

Engine.png_deflate (spa_png_deflate_u8, csrc/spa_png.hip) leaves one raw deflate stream and the Adler-32 of the
filtered scanlines per image; `assemble` adds what makes that a PNG file: the signature, IHDR, one IDAT holding the
zlib header, the stream and the Adler trailer, and IEND -- 57 bytes of PNG framing and 6 of zlib's, on the host.
What is pinned is the pixels a PNG reader gets back and, between the device and `deflate_rle_host`, the stream's
bytes; the bytes of Pillow's (or OpenCV's) files are not: another encoder, another stream.

deflate_rle_host is the plain numpy / Python restatement of the format fixed in include/spalign.h, written for the
tests; it is never on a product path.  nearest_tables is cv.INTER_NEAREST's index arithmetic (cli.resize_nearest),
held here once for the host resize and for the tables the encoder gathers through.  DeviceEncoder is what the batch
loops use: devenc.Ring, the buffer ring of every device encoder, with this module's bound, engine call and framing.
"""
import struct
import zlib

import numpy as np

from . import devenc

SIGNATURE = b'\x89PNG\r\n\x1a\n'
FRAMING_BYTES = 8 + (12 + 13) + 12 + 12                  # signature, IHDR, IDAT's length / tag / CRC, IEND = 57
ZLIB_BYTES = 2 + 4                                       # inside IDAT: the zlib header 78 01 and the Adler-32 trailer
IDAT_MAX = (1 << 31) - 1                                 # a chunk's length field


def deflate_bound(H, W):
    """spa_png_deflate_bound: bytes that hold the stream of any (H, W) image"""
    if H <= 0 or W <= 0:
        return 0
    return (3 + 9 * (W + 1) * H + 7 + 7) // 8


def nearest_index(n_dst, n_src):
    """source index of every destination index under cv.INTER_NEAREST: min(floor(dst * src/dst), src - 1)"""
    return np.minimum((np.arange(n_dst) * (n_src / n_dst)).astype(np.int64), n_src - 1)


def nearest_tables(src_shape, dst_shape):
    """(rows (dst H), columns (dst W)) int64: a[rows][:, columns] is cv.resize(a, INTER_NEAREST) to dst_shape"""
    return nearest_index(int(dst_shape[0]), int(src_shape[0])), nearest_index(int(dst_shape[1]), int(src_shape[1]))


def _chunk(tag, body):
    return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body) & 0xffffffff)


def assemble(deflate_bytes, adler, H, W):
    """the PNG file of an (H, W) 8-bit greyscale image from its raw deflate stream and the Adler-32 of its filtered
    scanlines: signature, IHDR (bit depth 8, colour type 0, no interlace), one IDAT = 78 01 + stream + big-endian
    Adler, IEND"""
    body = b'\x78\x01' + bytes(deflate_bytes) + struct.pack('>I', int(adler) & 0xffffffff)
    if len(body) > IDAT_MAX:
        raise ValueError('png.assemble: %d bytes do not fit one IDAT chunk' % len(body))
    return (SIGNATURE + _chunk(b'IHDR', struct.pack('>IIBBBBB', int(W), int(H), 8, 0, 0, 0, 0)) +
            _chunk(b'IDAT', body) + _chunk(b'IEND', b''))


def filtered_scanlines(img):
    """the bytes deflate sees: per row the filter type 2 (Up), then img[y] - img[y-1] mod 256 (row -1: zeros)"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape
    up = np.concatenate([np.zeros((1, W), np.uint8), img[:-1]], axis=0)
    rows = np.empty((H, W + 1), np.uint8)
    rows[:, 0] = 2
    rows[:, 1:] = img - up                               # uint8 arithmetic wraps: mod 256
    return rows


class _Bits(object):
    """deflate's bit order: bits fill a byte from its least-significant end"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        """nbits of value, least-significant first (extra bits, header fields)"""
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, nbits):
        """a Huffman code: most-significant bit first"""
        self.put(int(format(code, '0%db' % nbits)[::-1], 2), nbits)

    def finish(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def _symbol(bits, sym):
    """RFC 1951 3.2.6, the fixed literal/length code"""
    if sym < 144:
        bits.put_code(0x30 + sym, 8)
    elif sym < 256:
        bits.put_code(0x190 + sym - 144, 9)
    elif sym < 280:
        bits.put_code(sym - 256, 7)
    else:
        bits.put_code(0xC0 + sym - 280, 8)


# RFC 1951 3.2.5: (symbol, extra bits, first length) of the length codes
_LENGTHS = [(257 + i, 0, 3 + i) for i in range(8)] + \
           [(265 + 4 * (e - 1) + k, e, 3 + (4 + k) * (1 << e)) for e in range(1, 6) for k in range(4)] + [(285, 0, 258)]


def _match(bits, length):
    """a match of `length` (3..258) at distance 1"""
    sym, extra, base = [t for t in _LENGTHS if t[2] <= length][-1]
    assert 0 <= length - base < (1 << extra)
    _symbol(bits, sym)
    bits.put(length - base, extra)
    bits.put_code(0, 5)                                  # distance code 0: distance 1, no extra bits


def deflate_rle_host(img, row_idx=None, col_idx=None):
    """(H,W) uint8 (through the nearest-neighbour tables, if any) -> (raw deflate stream, Adler-32 of the filtered
    scanlines), the bytes spa_png_deflate_u8 writes."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError('deflate_rle_host: an (H, W) uint8 image, got %s %s' % (img.shape, img.dtype))
    if row_idx is not None:
        img = img[np.asarray(row_idx, dtype=np.int64)]
    if col_idx is not None:
        img = img[:, np.asarray(col_idx, dtype=np.int64)]
    rows = filtered_scanlines(img)
    bits = _Bits()
    bits.put(1, 1)                                       # BFINAL
    bits.put(1, 2)                                       # BTYPE = 01, fixed Huffman
    for row in rows:
        line = row.tolist()
        # maximal runs of equal bytes within the scanline
        edges = [0] + [i for i in range(1, len(line)) if line[i] != line[i - 1]] + [len(line)]
        for lo, hi in zip(edges[:-1], edges[1:]):
            v, r = line[lo], hi - lo - 1
            _symbol(bits, v)
            while r >= 3:
                length = min(r, 258)
                _match(bits, length)
                r -= length
            for _ in range(r):
                _symbol(bits, v)
    _symbol(bits, 256)
    return bits.finish(), zlib.adler32(rows.tobytes()) & 0xffffffff


class DeviceEncoder(devenc.Ring):
    """devenc.Ring for label PNGs from device masks: encode(masks) leaves the streams of masks (n,Hs,Ws) uint8 at
    `shape` (nearest resize inside the encoder) with their lengths and Adler sums, file_bytes(slot, j) is image j's
    PNG file.  pinned_bytes: the ring's first pinned buffer; by default every row's bound, so that none follows."""

    def __init__(self, engine, shape, batch, pinned_bytes=None):
        self.shape = (int(shape[0]), int(shape[1]))
        bound = deflate_bound(*self.shape)
        if bound + ZLIB_BYTES > IDAT_MAX:
            raise ValueError('png.DeviceEncoder: the payload of a %d x %d image may not fit one IDAT chunk' % self.shape)
        if pinned_bytes is None:
            pinned_bytes = max(int(batch), 1) * ((bound + 15) // 16 * 16)
        devenc.Ring.__init__(self, engine, batch, bound, 2, pinned_bytes)

    def launch(self, slot, masks, n):
        self.eng.png_deflate(masks, self.shape, out=slot['out'][:n], nbytes=slot['meta'][0, :n],
                             adler=slot['meta'][1, :n])

    def frame(self, slot, j, payload):
        return assemble(payload, slot['rows'][1][j] & 0xffffffff, self.shape[0], self.shape[1])


def write_file(fn, data):
    with open(fn, 'wb') as f:
        f.write(data)
