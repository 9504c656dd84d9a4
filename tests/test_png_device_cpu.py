"""The host side of --png_encoder device, without a GPU: png.deflate_rle_host (the restatement of the stream that
spa_png_deflate_u8 writes) and png.assemble on the images of png_cases.py.  Every file must be the image to Pillow, its
IDAT body the Up-filtered scanlines to zlib (which checks the Adler-32) and to a strict RFC 1951 reader, within
spa_png_deflate_bound, in exactly the chunks IHDR, IDAT, IEND (png_cases.check_file).  Three mutants of the restatement
show that the check can fail: runs that continue into the next scanline, Huffman codes written least-significant bit
first, and a match of 258 written as code 284 with 31 extra bits.  zlib and Pillow READ the third one as 258 (measured
here: zlib's inflate adds base and extra bits without a range check), so that one is caught by the strict reader alone;
the other two are refused by zlib as well."""
import importlib
import zlib

import numpy as np
import pytest

import png_cases

png = importlib.import_module('superpixel-align_amd.png')
CASES = png_cases.cases()


def resized(src, out_shape):
    """[(image as the encoder sees it, row table, column table)] of one case"""
    rows = cols = None
    if out_shape is not None:
        rows, cols = png.nearest_tables(src.shape[1:], out_shape)
    return [(im if rows is None else im[rows][:, cols], rows, cols) for im in src]


@pytest.mark.parametrize('name,src,out_shape', CASES, ids=[c[0] for c in CASES])
def test_restatement_makes_png_files_of_the_image(name, src, out_shape):
    for (img, rows, cols), im in zip(resized(src, out_shape), src):
        stream, adler = png.deflate_rle_host(im, rows, cols)
        assert len(stream) <= png.deflate_bound(*img.shape)
        assert adler == zlib.adler32(png.filtered_scanlines(img).tobytes())
        data = png.assemble(stream, adler, img.shape[0], img.shape[1])
        assert png.FRAMING_BYTES == 57 and len(data) == len(stream) + 57 + png.ZLIB_BYTES
        png_cases.check_file(png, data, img)


def test_bound_is_reached_by_nothing_and_refuses_nothing_small():
    assert png.deflate_bound(1, 1) == (3 + 18 + 7 + 7) // 8 and png.deflate_bound(0, 5) == 0
    assert png.deflate_bound(1024, 2048) == (3 + 9 * 2049 * 1024 + 14) // 8
    with pytest.raises(ValueError):
        png.deflate_rle_host(np.zeros((2, 2), np.int32))


def test_both_parsers_default_to_pillow_and_accept_device():
    cli = importlib.import_module('superpixel-align_amd.cli')
    dv = importlib.import_module('superpixel-align_amd.demovideo')
    assert cli.get_args_labelfree([]).png_encoder == 'pillow'
    assert cli.get_args_labelfree(['--png_encoder', 'device']).png_encoder == 'device'
    assert dv.demovideo_parser().parse_args([]).png_encoder == 'pillow'
    assert dv.demovideo_parser().parse_args(['--png_encoder', 'device']).png_encoder == 'device'
    for parse in (cli.get_args_labelfree, dv.demovideo_parser().parse_args):
        with pytest.raises(SystemExit):
            parse(['--png_encoder', 'zlib'])


@pytest.mark.parametrize('src,dst', png_cases.NEAREST)
def test_nearest_tables_are_resize_nearest(src, dst):
    cli = importlib.import_module('superpixel-align_amd.cli')
    # an image whose every pixel is its own index: the resized image IS the table
    a = np.arange(src[0] * src[1], dtype=np.int64).reshape(src)
    rows, cols = png.nearest_tables(src, dst)
    assert rows.shape == (dst[0],) and cols.shape == (dst[1],)
    assert np.array_equal(cli.resize_nearest(a, dst), rows[:, None] * src[1] + cols[None, :])
    # cli.py's rule, written out
    assert np.array_equal(rows, np.minimum((np.arange(dst[0]) * (src[0] / dst[0])).astype(np.int64), src[0] - 1))
    assert np.array_equal(cols, np.minimum((np.arange(dst[1]) * (src[1] / dst[1])).astype(np.int64), src[1] - 1))
    assert np.array_equal(cli.nearest_index(dst[0], src[0]), rows)


# ------------------------------------------------------------------------------- mutants
def runs_across_scanlines(img):
    """the restatement with one change: a scanline's first run, when it has the value the scanline above ended with,
    is written as the continuation of that run (matches and literals, no opening literal) -- behind the filter byte a
    match at distance 1 copies the 2, not the value"""
    rows = png.filtered_scanlines(img)
    bits = png._Bits()
    bits.put(1, 1)
    bits.put(1, 2)
    last = None
    for row in rows:
        line = row.tolist()
        png._symbol(bits, line[0])
        body = line[1:]
        edges = [0] + [i for i in range(1, len(body)) if body[i] != body[i - 1]] + [len(body)]
        for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
            v, r = body[lo], hi - lo
            if not (k == 0 and v == last):
                png._symbol(bits, v)
                r -= 1
            while r >= 3:
                length = min(r, 258)
                png._match(bits, length)
                r -= length
            for _ in range(r):
                png._symbol(bits, v)
        last = body[-1]
    png._symbol(bits, 256)
    return bits.finish(), zlib.adler32(rows.tobytes())


def test_the_check_rejects_three_mutants(monkeypatch):
    img = np.zeros((3, 600), np.uint8)                             # every scanline: 2, then 600 zeros = 258 + 258 + 83
    img[1:, 300:] = 9
    good = png.assemble(*png.deflate_rle_host(img), 3, 600)
    png_cases.check_file(png, good, img)

    stream, adler = runs_across_scanlines(img)
    with pytest.raises((zlib.error, AssertionError)):
        png_cases.check_file(png, png.assemble(stream, adler, 3, 600), img)

    with monkeypatch.context() as m:
        m.setattr(png._Bits, 'put_code', lambda self, code, nbits: self.put(code, nbits))
        stream, adler = png.deflate_rle_host(img)
    assert stream != png.deflate_rle_host(img)[0]
    with pytest.raises((zlib.error, AssertionError)):
        png_cases.check_file(png, png.assemble(stream, adler, 3, 600), img)

    with monkeypatch.context() as m:
        m.setattr(png, '_LENGTHS', png._LENGTHS[:-1])               # no code 285: 258 becomes 284 + 31
        stream, adler = png.deflate_rle_host(img)
    assert stream != png.deflate_rle_host(img)[0]
    with pytest.raises(png_cases.StreamError, match='284'):
        png_cases.check_file(png, png.assemble(stream, adler, 3, 600), img)
    png_cases.check_file(png, good, img)                           # the patches are gone
