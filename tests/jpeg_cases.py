"""The frames that the JPEG tests encode, and what they share: the restart intervals to try, Pillow's own quality-75
file as the yardstick, PSNR, and a reader of a JPEG file's segments.  Each case is (name, frame (H,W,3) uint8); the
shapes are 16x16 (one MCU), 16x32, 32x48, 48x80 and 64x96, small enough for the Python restatement and chosen so that
the list as a whole reaches every branch of the entropy coder (test_jpeg_device_cpu.py counts them):

  edge       16x16  every 8x8 block white on its left half and black on its right: the largest AC category (8)
  chroma     16x32  colour noise in 2x2 cells, so the chrominance blocks keep their noise: a chrominance block without
                    EOB ends an interval in 1-bits, and the padded byte is 0xFF and stuffed
  checker    32x48  a pixel checkerboard: coefficient 63 of every luminance block, long runs of 1-bits
  noise      48x80  uniform noise: ZRL, blocks without EOB, stuffed bytes
  mcus       64x96  every MCU black or white: DC differences of +-255, the largest category (8); 24 MCUs, so Ri = 1
                    wraps the RST index three times
  smooth     64x96  a colour gradient, what a photograph mostly is
"""
import io
import math
import struct
import warnings

import numpy as np


def edge():
    row = np.where(np.arange(16) % 8 < 4, 255, 0).astype(np.uint8)
    return np.broadcast_to(row[None, :, None], (16, 16, 3)).copy()


def chroma():
    return np.random.default_rng(0).integers(0, 256, (8, 16, 3), dtype=np.uint8).repeat(2, 0).repeat(2, 1)


def checker():
    y, x = np.indices((32, 48))
    return np.broadcast_to((((y + x) & 1) * 255).astype(np.uint8)[:, :, None], (32, 48, 3)).copy()


def noise(seed=1, shape=(48, 80)):
    return np.random.default_rng(seed).integers(0, 256, shape + (3,), dtype=np.uint8)


def mcus():
    cells = np.random.default_rng(2).integers(0, 2, (4, 6)).astype(np.uint8) * 255
    cells[0, :4] = (0, 255, 0, 255)                      # both signs, whatever the generator gives
    return np.broadcast_to(cells.repeat(16, 0).repeat(16, 1)[:, :, None], (64, 96, 3)).copy()


def smooth(shape=(64, 96)):
    y, x = np.indices(shape)
    return np.stack([(2 * y + x) % 256, (2 * x) % 256, (3 * y) % 256], axis=-1).astype(np.uint8)


def cases():
    return [('edge', edge()), ('chroma', chroma()), ('checker', checker()), ('noise', noise()), ('mcus', mcus()),
            ('smooth', smooth())]


def intervals_for(frame):
    """the restart intervals every case is tried at: 1, 3, one MCU row, and one that holds the whole frame (each once
    where two of them are the same number)"""
    H, W = frame.shape[:2]
    n_mcu = (H // 16) * (W // 16)
    return list(dict.fromkeys([1, 3, W // 16, n_mcu + 5]))


def pillow_jpeg(frame, quality=75):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format='JPEG', quality=quality)
    return buf.getvalue()


def decode(data):
    """the file through Pillow with every warning an error -> (H,W,3) uint8"""
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        with Image.open(io.BytesIO(data)) as f:
            assert f.format == 'JPEG' and f.mode == 'RGB', (f.format, f.mode)
            f.load()
            return np.asarray(f.convert('RGB'), dtype=np.uint8)


def psnr(a, b):
    mse = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())
    return math.inf if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def segments(data):
    """[(marker, body)] of a JPEG file up to and including SOS"""
    assert data[:2] == b'\xff\xd8'
    out, p = [], 2
    while True:
        assert data[p] == 0xFF, p
        marker, n = data[p + 1], struct.unpack('>H', data[p + 2:p + 4])[0]
        out.append((marker, data[p + 4:p + 2 + n]))
        p += 2 + n
        if marker == 0xDA:
            return out, p
