"""CPU: the format of a small image's file (HOH_OPT_SMALL_IMAGES).

The reference's choh codes the single tile of an untiled image, throws the bytes away and writes
the header alone (choh.cpp:508-520); its dhoh calls decode_tile right after the header
(dhoh.cpp:379).  So the file a small image should have is header || encode_tile(whole image), and
its length is the number choh prints.  Pinned here with the oracle alone: for every shape,
len(choh file) + len(encode_tile) == printed, the choh file is the header, and or_decode_tile reads
a sub-green tile back behind it."""
import ctypes as C

import numpy as np
import pytest

from hoh_ans.natural import natural_rgb
from hoh_ans.synth import synth_rgb

SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (63, 65), (64, 64), (65, 63), (200, 100), (255, 255), (256, 256),
          (385, 300), (300, 511), (511, 511)]


def header(W, H):
    def vi(v):
        return bytes([v]) if v < 128 else bytes([(v >> 7) + 128, v % 128])
    return bytes([153, 72, 79, 72, 2, 8]) + vi(W - 1) + vi(H - 1)


def decode_tile(orc, data, p, w, h):
    L = orc.lib()
    L.or_decode_tile.restype = C.c_long
    L.or_decode_tile.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    out = np.empty((h, w, 3), np.uint8)
    r = L.or_decode_tile(bytes(data), len(data), p, w, h, out.ctypes.data)
    return r, out


def _images(W, H):
    return [("noise3", synth_rgb(W, H, 5, 3)), ("noise0", synth_rgb(W, H, 6, 0))]


@pytest.mark.parametrize("W,H", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("speed", [0, 2])
def test_file_plus_tile_is_printed(orc, W, H, speed):
    for name, img in _images(W, H):
        data, printed = orc.choh(img, speed)
        assert data == header(W, H), name
        try:
            tile = orc.encode_tile(img, speed)
        except orc.OracleError:
            continue                                  # non-binary grey: the reference's bytes are undefined
        assert tile[:2] == b"\0\0"                    # the tile's own 1x1 tiling (choh.cpp:115-116)
        assert len(data) + len(tile) == printed, (name, len(data), len(tile), printed)
        if speed == 0 and tile[2] == 128:
            r, back = decode_tile(orc, data + tile, len(data), W, H)
            assert r >= 0 and np.array_equal(back, img), name


@pytest.mark.parametrize("W,H", [(224, 224), (511, 300)])
def test_natural_crops(orc, W, H):
    img = natural_rgb(W, H, 3)
    data, printed = orc.choh(img, 0)
    tile = orc.encode_tile(img, 0)
    assert data == header(W, H) and len(data) + len(tile) == printed
    r, back = decode_tile(orc, data + tile, len(data), W, H)
    assert r >= 0 and np.array_equal(back, img)


def test_tiny_tiles_are_palette(orc):
    """1x1 .. 3x5 hold at most 15 colours: the reference takes the indexed mode (127), which carries
    no palette (Q15) and cannot be decoded"""
    for W, H in SHAPES[:5]:
        assert orc.encode_tile(synth_rgb(W, H, 5, 3), 0)[2] == 127, (W, H)
