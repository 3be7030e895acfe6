"""hoh_region_cover (host only): the tile rectangle of a pixel window, against a brute force over
hoh_tiling that marks every tile holding a pixel of the window; its status codes; and the region
decode entry points' presence in the header and the library."""
import ctypes as C
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = 1, 6


@pytest.fixture(scope="module")
def hoh():
    import hoh_ans
    return hoh_ans


def _grid(hoh, W, H):
    tiled, xt, yt, tw, th = hoh.tiling(W, H)
    assert tiled
    # tile column i holds pixels [xs[i], xs[i + 1]) (choh.cpp:464-500: the last one may be narrower)
    xs = [min(W, i * tw) for i in range(xt)] + [W]
    ys = [min(H, i * th) for i in range(yt)] + [H]
    return xs, ys


def _brute(xs, ys, x, y, w, h):
    """(tx0, ty0, ntx, nty) from the tiles that hold any pixel of [x, x+w) x [y, y+h)"""
    cols = [i for i in range(len(xs) - 1) if xs[i] < x + w and xs[i + 1] > x]
    rows = [i for i in range(len(ys) - 1) if ys[i] < y + h and ys[i + 1] > y]
    assert cols == list(range(cols[0], cols[-1] + 1)) and rows == list(range(rows[0], rows[-1] + 1))
    return cols[0], rows[0], len(cols), len(rows)


def _edges(n, seams, step):
    """corner coordinates in [0, n]: a coarse grid plus every tile seam and its neighbours"""
    pts = set(range(0, n + 1, step)) | {n}
    for s in seams:
        pts |= {s - 1, s, s + 1}
    return sorted(p for p in pts if 0 <= p <= n)


@pytest.mark.parametrize("W,H,step", [(768, 512, 97), (1000, 600, 131)])
def test_cover_matches_brute_force_small(hoh, W, H, step):
    xs, ys = _grid(hoh, W, H)
    ex, ey = _edges(W, xs, step), _edges(H, ys, step)
    n = 0
    for x0 in ex:
        for x1 in ex:
            if x1 <= x0:
                continue
            for y0 in ey:
                for y1 in ey:
                    if y1 <= y0:
                        continue
                    got = hoh.region_cover(W, H, x0, y0, x1 - x0, y1 - y0)
                    assert got == _brute(xs, ys, x0, y0, x1 - x0, y1 - y0), (x0, y0, x1, y1)
                    n += 1
    assert n > 1000


def test_cover_matches_brute_force_8192(hoh):
    W = H = 8192
    xs, ys = _grid(hoh, W, H)
    rng = random.Random(8192)
    for _ in range(400):
        w, h = rng.randint(1, W), rng.randint(1, H)
        if rng.random() < 0.5:
            w, h = rng.randint(1, 600), rng.randint(1, 600)
        x, y = rng.randint(0, W - w), rng.randint(0, H - h)
        assert hoh.region_cover(W, H, x, y, w, h) == _brute(xs, ys, x, y, w, h), (x, y, w, h)
    assert hoh.region_cover(W, H, 3000, 3000, 512, 512) == (11, 11, 3, 3)
    assert hoh.region_cover(W, H, 0, 0, W, H) == (0, 0, 32, 32)


def test_cover_status_codes(hoh):
    W, H = 768, 512

    def code(*a):
        with pytest.raises(hoh.HohError) as e:
            hoh.region_cover(*a)
        return e.value.code

    for bad in [(0, 0, 0, 5), (0, 0, 5, 0), (0, 0, -1, 5), (0, 0, 5, -1), (-1, 0, 5, 5), (0, -1, 5, 5),
                (W - 4, 0, 5, 5), (0, H - 4, 5, 5), (W, 0, 1, 1), (0, H, 1, 1), (0, 0, W + 1, 1), (0, 0, 1, H + 1),
                (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)]:
        assert code(W, H, *bad) == E_ARG, bad
    assert code(0, 512, 0, 0, 1, 1) == E_ARG
    assert code(300, 300, 0, 0, 10, 10) == E_UNSUPPORTED         # an untiled shape
    assert code(300, 300, 0, 0, 0, 10) == E_ARG                   # the rectangle is judged first
    assert hoh.region_cover(W, H, W - 1, H - 1, 1, 1) == (2, 1, 1, 1)


def test_region_entry_points_declared_and_exported(hoh):
    with open(os.path.join(ROOT, "include", "hoh_ans.h")) as f:
        hdr = f.read()
    L = C.CDLL(hoh.LIBPATH)
    for name in ("hoh_region_cover", "hoh_decode_region", "hoh_decode_region_async", "hoh_decode_regions_async"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
    assert re.search(r"#define\s+HOH_REGION_MAX_BATCH\s+256\b", hdr)
    for fn in ("region_cover", "decode_region", "decode_region_async", "decode_regions_async"):
        assert callable(getattr(hoh, fn))
