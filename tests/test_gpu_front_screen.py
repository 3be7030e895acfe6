"""GPU: k_front256's two-mode LZ candidate screen (bit-filter fast path, table mode for dense repeats).

Every image is 512 x 512 or smaller with sides that are multiples of 256, so every tile is a full
256 x 256 tile.  The base image is synth_rgb(noise=40): repeat-free, far from palette and grey
tiles.  Repeats are pasted in raster order of the *tile* (a window may wrap from a row's end to the
next row's start).

* file parity with the oracle (product library and checking build);
* the exact candidate set: the candidate bitmap and each tile's ncand, read back from the checking
  build, equal a numpy recomputation of the definition (position q is a candidate iff q + 3 < npix
  and the window q..q+3 equals the window at q - b for some 1 <= b <= min(q, 64)): equality, not
  only a superset (a superset would be byte-safe but would move work into k_lz);
* the same under the forcing knobs (a 64-bit filter, which flags nearly every chunk so that both
  resolutions run constantly; each mode pinned), each in a process of its own (knobs are read once);
* determinism: four encodes of the natural image give identical bytes."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "hoh-ans_amd")):      # the knob children import this module
    if _p not in sys.path:
        sys.path.insert(0, _p)

T = 256
NPIX = T * T
TILE_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("colours", "<i4"), ("flags", "<u4"),
                       ("nmatch", "<u4"), ("ncand", "<u4"), ("size", "<u4"), ("lz_bytes", "<u4"), ("off", "<u8"),
                       ("mode", "<u4"), ("pad", "<u4"), ("nclean", "<u4"), ("nfut", "<u4"), ("chmap", "<u4"),
                       ("pad2", "<u4")])          # TileInfo (hoh-ans_amd/csrc/hoh_internal.h)
assert TILE_DTYPE.itemsize == 72


def tiles_of(img):
    """the image's tiles in tile order, each as a (65536, 3) array in tile raster order (copies)"""
    H, W = img.shape[:2]
    return [img[y:y + T, x:x + T].reshape(NPIX, 3).copy() for y in range(0, H, T) for x in range(0, W, T)]


def put_tiles(img, tiles):
    H, W = img.shape[:2]
    k = 0
    for y in range(0, H, T):
        for x in range(0, W, T):
            img[y:y + T, x:x + T] = tiles[k].reshape(T, T, 3)
            k += 1


def paste(tile, p, L, b):
    """an LZ repeat of length L at back distance b starting at tile raster position p"""
    for i in range(L):
        tile[p + i] = tile[p + i - b]


def base(W, H, seed):
    from hoh_ans.synth import synth_rgb
    return synth_rgb(W, H, seed, 40)


def cases():
    out = []
    # lengths 4, 5 and 70 at each back distance 1..64 (one length per tile, start lanes vary);
    # the fourth tile: length 3 at any distance and length 4 at distance 65 (neither is a candidate)
    img = base(512, 512, 21)
    ts = tiles_of(img)
    for k, L in enumerate((4, 5, 70)):
        for b in range(1, 65):
            paste(ts[k], 301 + b * 1003, L, b)
    for b in range(1, 65):
        paste(ts[3], 301 + b * 1003, 3, b)
        paste(ts[3], 801 + b * 1003, 4, 65)
    put_tiles(img, ts)
    out.append(("distances", img))
    # window positions: chunk crossings, row ends, stripe boundaries, the tile's start and end
    img = base(512, 512, 22)
    ts = tiles_of(img)
    for n, lane in enumerate((60, 61, 62, 63)):           # starts in lanes 60..63: the window crosses the chunk
        for m, b in enumerate((1, 3, 17, 61, 64)):
            paste(ts[0], 64 * (40 + 10 * (5 * n + m)) + lane, 4 + m, b)
    for n, x in enumerate((253, 254, 255)):               # crossing a row end
        paste(ts[0], 256 * (100 + 3 * n) + x, 6, 2 + 30 * n)
    for row in (64, 128, 192):                            # crossing the stripe boundaries 63/64, 127/128, 191/192
        paste(ts[1], 256 * row - 2, 4, 9)                 # the window straddles the boundary
        paste(ts[1], 256 * row + 70, 4, 64)
        paste(ts[2], 256 * row, 5, 1)                     # the stripe's first window, source in the stripe above
        paste(ts[2], 256 * row + 10, 4, 64)
        paste(ts[3], 256 * row - 3, 70, 33)
    paste(ts[0], 1, 4, 1)                                 # the first 64 positions: fewer than 64 lie behind
    paste(ts[0], 20, 4, 11)
    paste(ts[1], 40, 5, 40)
    paste(ts[1], 59, 8, 33)
    paste(ts[2], 63, 4, 63)
    paste(ts[3], 7, 60, 7)
    paste(ts[2], NPIX - 4, 4, 17)                         # the window ends on the tile's last pixel
    paste(ts[3], NPIX - 5, 5, 23)                         # ... and one past it (no window at NPIX - 3)
    paste(ts[1], NPIX - 3, 3, 5)
    put_tiles(img, ts)
    out.append(("positions", img))
    # bands of rows with period-1, -2, -3, -5 and -64 pixel patterns alternating with noise bands
    # every few rows (switches in both directions); with 4 + 4 rows a band edge falls on every
    # stripe's first chunk (rows 64, 128, 192), with 3 + 3 rows edges fall inside the stripes
    img = base(512, 512, 23)
    rs = np.random.RandomState(3)
    ts = tiles_of(img)
    for k in range(4):
        cyc = (8, 6, 8, 10)[k]
        for n, r in enumerate(range(0 if k != 2 else 4, T, cyc)):
            per = (1, 2, 3, 5, 64)[n % 5]
            pal = rs.randint(0, 256, (per, 3)).astype(np.uint8)
            rows = min(cyc // 2, T - r)
            ts[k][r * T:(r + rows) * T] = pal[np.arange(rows * T) % T % per]
    put_tiles(img, ts)
    out.append(("bands", img))
    from hoh_ans.natural import natural_rgb
    out.append(("natural", natural_rgb(512, 512, 1)))
    return out


def candidates(tile):
    """the definition: bool per position of a (65536, 3) tile"""
    px = tile[:, 0].astype(np.uint32) | tile[:, 1].astype(np.uint32) << 8 | tile[:, 2].astype(np.uint32) << 16
    n = len(px)
    c = np.zeros(n, bool)
    for b in range(1, 65):
        e = px[b:] == px[:-b]                             # e[i]: pixel b + i equals pixel i
        c[b:n - 3] |= e[:-3] & e[1:-2] & e[2:-1] & e[3:]
    return c


def want_bits(img):
    """(candidate words [tile][1024] u64, ncand per tile)"""
    cs = [candidates(t) for t in tiles_of(img)]
    words = np.stack([np.packbits(c, bitorder="little").view("<u8") for c in cs])
    return words, np.array([int(c.sum()) for c in cs])


_CASES = None
_REF = {}


def the_cases():
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


def ref_file(orc, name, img):
    if name not in _REF:
        _REF[name] = orc.choh(img)
    return _REF[name]


def check_encode(c, torch, img):
    """encode with the checking build -> (file bytes, candidate words, ncand per tile)"""
    H, W = img.shape[:2]
    nt = (W // T) * (H // T)
    f = c.encode(torch.from_numpy(np.ascontiguousarray(img)).cuda().reshape(-1), W, H, 0, torch)
    bits = c.read(7, np.zeros(nt * (NPIX // 64), np.uint64)).reshape(nt, NPIX // 64)
    ti = c.read(8, np.zeros(nt, TILE_DTYPE))
    return f, bits, ti["ncand"].astype(np.int64)


def describe(bits, want):
    d = bits ^ want
    t, w = np.argwhere(d != 0)[0]
    lanes = [i for i in range(64) if (int(d[t, w]) >> i) & 1]
    return "tile %d chunk %d (row %d) lanes %s: got %016x want %016x; %d words differ" % (
        t, w, w // 4, lanes, int(bits[t, w]), int(want[t, w]), int((d != 0).sum()))


def test_cases_have_what_they_claim():
    """the numpy definition on the pasted images: candidates exist where pasted, not where not"""
    cs = dict(the_cases())
    ts = tiles_of(cs["distances"])
    for k, L in enumerate((4, 5, 70)):
        c = candidates(ts[k])
        assert int(c.sum()) == 64 * (L - 3), (L, int(c.sum()))
        assert all(c[301 + b * 1003] for b in range(1, 65))
    assert not candidates(ts[3]).any()
    ts = tiles_of(cs["positions"])
    c2, c3, c1 = candidates(ts[2]), candidates(ts[3]), candidates(ts[1])
    assert c2[NPIX - 4] and c3[NPIX - 5] and c3[NPIX - 4] and not c1[NPIX - 6:].any()
    assert candidates(ts[0])[1] and c2[63] and c2[256 * 64] and c1[256 * 64 - 2]
    words, ncand = want_bits(cs["bands"])
    assert (ncand > 20000).all() and ((words == 0).sum(axis=1) > 300).all()     # dense bands and clean chunks
    assert base(512, 512, 21).shape == (512, 512, 3) and not any(candidates(t).any() for t in tiles_of(base(512, 512, 21)))


@pytest.mark.parametrize("name", ["distances", "positions", "bands", "natural"])
def test_product_parity(orc, name):
    import hoh_ans
    img = dict(the_cases())[name]
    ref, ref_printed = ref_file(orc, name, img)
    data, printed = hoh_ans.choh(img)
    assert len(data) == len(ref)
    assert data == ref
    assert printed == ref_printed


def test_exact_candidates_and_parity_check_build(orc):
    import torch
    from checklib import CheckLib
    c = CheckLib()
    try:
        for name, img in the_cases():
            f, bits, ncand = check_encode(c, torch, img)
            want, wn = want_bits(img)
            assert np.array_equal(bits, want), (name, describe(bits, want))
            assert np.array_equal(ncand, wn), (name, ncand.tolist(), wn.tolist())
            assert f == ref_file(orc, name, img)[0], name
    finally:
        c.close()


_KNOB_CHILD = r"""
import hashlib, json, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import test_gpu_front_screen as S
from checklib import CheckLib
c = CheckLib()
res = {}
for name, img in S.the_cases():
    f, bits, ncand = S.check_encode(c, torch, img)
    want, wn = S.want_bits(img)
    ok = bool(np.array_equal(bits, want))
    dbg = c.read(5, np.zeros(len(wn) * 64, np.uint32)).reshape(-1, 64)[:, 56:61].sum(axis=0)
    res[name] = {"sha": hashlib.sha256(f).hexdigest(), "bits": ok, "ncand": bool(np.array_equal(ncand, wn)),
                 "what": "" if ok else S.describe(bits, want), "modes": dbg.tolist()}
c.close()
print("RESULT " + json.dumps(res))
"""

# a 64-bit filter (two words, each lane sets two bits of one) is nearly full after a chunk, so
# most of a chunk's 64 lanes are flagged: with the product's threshold every chunk enters table
# mode (and noise leaves it again); with a threshold of 61 most noise chunks are resolved lane by
# lane on the fast path instead and the denser ones still switch
KNOBS = {"filter64": {"HOH_F2_MLOG2": "6"}, "filter64-thr61": {"HOH_F2_MLOG2": "6", "HOH_F2_THR": "61", "HOH_F2_QUIET": "2"},
         "fast-only": {"HOH_F2_MODE": "1"}, "table-only": {"HOH_F2_MODE": "2"}}


def test_exact_candidates_and_parity_under_knobs(orc):
    """every forcing knob in a process of its own, side by side"""
    want_sha = {name: hashlib.sha256(ref_file(orc, name, img)[0]).hexdigest() for name, img in the_cases()}
    procs = {k: subprocess.Popen([sys.executable, "-c", _KNOB_CHILD, HERE], env=dict(os.environ, HOH_QUIET="1", **env),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k, env in KNOBS.items()}
    outs = {k: p.communicate(timeout=100) + (p.returncode,) for k, p in procs.items()}
    for k, (so, se, rc) in outs.items():
        assert rc == 0, (k, se[-3000:])
        res = json.loads([ln for ln in so.splitlines() if ln.startswith("RESULT ")][-1][7:])
        for name, r in res.items():
            print(k, name, "clean/resolved/table chunks, switches to table/to fast:", r["modes"])
            assert r["bits"], (k, name, r["what"])
            assert r["ncand"], (k, name)
            assert r["sha"] == want_sha[name], (k, name)
        clean, resolved, table, to_tab, to_fast = np.sum([r["modes"] for r in res.values()], axis=0)
        if k == "fast-only":
            assert table == 0 and to_tab == 0 and resolved > 0
        if k == "table-only":
            assert clean == 0 and resolved == 0 and to_fast == 0 and table > 0
        if k == "filter64":
            assert to_tab > 1000 and to_fast > 1000                      # switches all the time
        if k == "filter64-thr61":
            assert resolved > 1000 and to_tab > 100 and to_fast > 100    # both resolutions ran


def test_determinism_natural():
    import hoh_ans
    img = dict(the_cases())["natural"]
    first = hoh_ans.choh(img)[0]
    for _ in range(3):
        assert hoh_ans.choh(img)[0] == first
