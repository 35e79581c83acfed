"""Writes tests/golden/gallery_*.png: a band of rows from each of the four gallery PNGs the upstream project ships
(rust_ray_tracing README images, 1920 wide, non-interlaced, 8-bit RGB / RGBA) -- the fixture of
tests/test_obj_loader.py::test_png_decoder_on_the_reference_gallery_images.

The band keeps the original encoder's output where it matters to a decoder: the width, the colour type, the ancillary
chunks and every row's filter byte and filtered bytes are copied as they are; only the deflate stream is redone (zlib,
level 9) over the shorter image and split into IDAT chunks of the original's size.  A band that starts below row 0
keeps its first row's Up / Average / Paeth filter, which a decoder then applies against a zero row, as the standard says.

    python tests/golden/make_gallery_bands.py <directory holding the upstream gallery PNGs>
"""
import glob
import os
import struct
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = 24


def chunks(data):
    i = 8
    while i < len(data):
        n, = struct.unpack(">I", data[i:i + 4])
        yield data[i + 4:i + 8], data[i + 8:i + 8 + n]
        i += 12 + n


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def band(src, dst):
    data = open(src, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", src
    parts = list(chunks(data))
    w, h, depth, ctype, comp, filt, interlace = struct.unpack(">IIBBBBB", parts[0][1])
    assert depth == 8 and ctype in (2, 6) and interlace == 0, src
    idat = [b for k, b in parts if k == b"IDAT"]
    raw = zlib.decompress(b"".join(idat))
    stride = 1 + w * (3 if ctype == 2 else 4)
    kinds = [raw[r * stride] for r in range(h)]
    # the band nearest the middle of the picture (geometry, not sky) whose rows use every filter type the image uses
    starts = sorted(range(h - ROWS + 1), key=lambda r: abs(r - h // 2))
    first = next((r for r in starts if set(kinds[r:r + ROWS]) == set(kinds)), h // 2)
    rows = raw[first * stride:(first + ROWS) * stride]
    z = zlib.compress(rows, 9)
    size = len(idat[0])
    out = [b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", w, ROWS, depth, ctype, comp, filt, interlace))]
    out += [chunk(k, b) for k, b in parts[1:] if k not in (b"IDAT", b"IEND")]
    out += [chunk(b"IDAT", z[i:i + size]) for i in range(0, len(z), size)]
    out.append(chunk(b"IEND", b""))
    open(dst, "wb").write(b"".join(out))


if __name__ == "__main__":
    for f in sorted(glob.glob(os.path.join(sys.argv[1], "*.png"))):
        band(f, os.path.join(HERE, "gallery_" + os.path.basename(f)))
