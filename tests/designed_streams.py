"""Tiles whose residual streams are chosen, not produced by an image: frequency tables and prob_bits
that no encoder of ours writes, in the -s0 tile shape (mode 128, three LZ streams, three 1x1 0x0010
layers) the decoder's chain kernels take.  Built from oracle primitives and tests/decodable_ref.py.

A design is a residual sequence.  An 8-bit design is the G plane's (any sequence is a plane:
unpredict_fastpath), with R = B = G so that the two 9-bit planes are single-symbol.  A 9-bit design
is the plane R' = R - G + 256 (or B'): its values must lie in 1..511, G is then chosen per pixel so
that R lands in 0..255, and the other colour follows G.  Where a value 0 would occur the residual
there is swapped with the next different one (the histogram is kept) and the plane recomputed.

rans_walk is a pure-Python model of the coder (rans64.hpp:107-142, 262-278) over the oracle's
normalised frequencies: it encodes backward, decodes forward and counts the payload words every
16-symbol group reads -- what the decoders' payload rings are sized by."""
import functools

import numpy as np

import decodable_ref as dr

S0 = [(1, 1, [0x0010], [0])] * 3
BURST_AT = 20 * 1024 + 777                                    # inside a 1024-symbol segment, runs over its end


def _orc():
    import oracle
    return oracle


# ------------------------------------------------------------------ the coder, step by step

def rans_walk(sym, rng, pb):
    """-> dict(freq, cum, words (u32, in the order the decoder reads them: the state first), groups
    (payload words read per 16-symbol group, aligned to the stream start))"""
    sym = np.asarray(sym, np.int64)
    f, c = _orc().normalize_freqs(np.bincount(sym, minlength=rng), 1 << pb)
    fl, cl, s = f.tolist(), c.tolist(), sym.tolist()
    x, rev = 1 << 31, []
    lim = ((1 << 31) >> pb) << 32
    for v in reversed(s):                                     # Rans64EncPutSymbol
        fv = fl[v]
        if x >= lim * fv:
            rev.append(x & 0xffffffff)
            x >>= 32
        x = ((x // fv) << pb) + x % fv + cl[v]
    rev += [x >> 32, x & 0xffffffff]                          # Rans64EncFlush
    words = rev[::-1]
    lut = np.repeat(np.arange(rng), f).tolist()
    mask = (1 << pb) - 1
    groups = [0] * ((len(s) + 15) // 16)
    x, wi = words[0] | (words[1] << 32), 2
    for i, want in enumerate(s):                              # Rans64DecAdvance
        slot = x & mask
        v = lut[slot]
        assert v == want, (i, v, want)
        x = fl[v] * (x >> pb) + slot - cl[v]
        if x < 1 << 31:
            x = (x << 32) | words[wi]
            wi += 1
            groups[i >> 4] += 1
    assert x == 1 << 31 and wi == len(words)
    return dict(freq=f, cum=c, words=np.array(words, "<u4"), groups=np.array(groups))


def bucket_starts(cum, pb):
    """symbol starts per 64-slot bucket, and the starts themselves"""
    cum = np.asarray(cum, np.int64)
    st = cum[:-1][np.diff(cum) > 0]
    return np.bincount(st >> 6, minlength=max(1, (1 << pb) >> 6)), st


# ------------------------------------------------------------------ residuals -> tiles

def tile8(res, w, h):
    orc = _orc()
    res = np.asarray(res, np.uint16)
    g = orc.unpredict_fastpath(res, w, h, 8)
    assert int(g.max()) < 256 and np.array_equal(orc.predict_fastpath(g, 8).reshape(-1), res)
    return np.stack([g, g, g], -1).astype(np.uint8), res


def tile9(res, w, h, plane):
    """plane 1: the design is R', 2: B'"""
    orc = _orc()
    res = np.array(res, np.uint16)
    for _ in range(8192):
        v = orc.unpredict_fastpath(res, w, h, 9).reshape(-1)
        z = np.flatnonzero(v == 0)
        if not z.size:
            break
        i = int(z[0])
        j = i + 1 + int(np.flatnonzero(res[i + 1:] != res[i])[0])
        res[i], res[j] = res[j], res[i]
    else:
        raise AssertionError("the plane keeps reaching 0")
    assert int(v.max()) < 512 and np.array_equal(orc.predict_fastpath(v.reshape(h, w), 9).reshape(-1), res)
    v = v.reshape(h, w).astype(np.int64)
    g = (511 - v) // 2                                        # the middle of the G that keep v - 256 + G in 0..255
    d = v - 256 + g
    assert d.min() >= 0 and d.max() <= 255
    px = np.stack([d if plane == 1 else g, g, d if plane == 2 else g], -1).astype(np.uint8)
    return px, res


# ------------------------------------------------------------------ the designs (residual sequences)

def d_two(n, half, other):
    r = np.full(n, half, np.uint16)
    r[n // 3 + 5] = other
    return r


def d_burst(n, rng, peak, rs, at=BURST_AT):
    """every symbol but the peak twice in a row (the pairs in random order) from `at` on"""
    others = np.array([s for s in range(rng) if s != peak])
    rs.shuffle(others)
    r = np.full(n, peak, np.uint16)
    r[at:at + 2 * others.size] = np.repeat(others, 2)
    return r


def d_equal(n, rng, rs):
    """half of the range's symbols, equally often, in random order"""
    syms = np.sort(rs.permutation(rng)[:rng // 2])
    r = np.repeat(syms, n // syms.size).astype(np.uint16)
    assert r.size == n
    rs.shuffle(r)
    return r


def d_geo(n, half, p, clip, rs):
    mag = rs.geometric(p, n) - 1
    return np.clip(half + mag * rs.choice([-1, 1], n), half - clip, half + clip).astype(np.uint16)


def d_full(n, rs):
    """P = 512: a geometric body and every symbol at least once"""
    r = np.clip(256 + (rs.geometric(0.05, n) - 1) * rs.choice([-1, 1], n), 0, 511).astype(np.uint16)
    r[rs.permutation(n)[:512]] = np.arange(512)
    return r


def _lz_tile(rs, periods):
    """every row repeats itself `period` pixels on (within reach of lz_distance 6); the pixels that
    are left take few values, so that their short streams still code as rANS"""
    px = np.zeros((256, 256, 3), np.uint8)
    for y, p in enumerate(periods):
        cell = 100 + rs.randint(0, 4, (p, 3))
        px[y] = np.tile(cell, (256 // p + 1, 1))[:256]
    return px


# ------------------------------------------------------------------ cases and files

def _case(name, design, depth, pb, px, res, pbs, plane, lz=None):
    tile = dr.build_tile(px, S0, lz_distance=lz, pbs=pbs)
    return dict(name=name, design=design, depth=depth, pb=pb, plane=plane, px=px, res=res, pbs=pbs, tile=tile)


def _other(pbs, plane, pb):
    """the designed plane at pb, the other two at the prob_bits given"""
    out = list(pbs)
    out[plane] = pb
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: the tile's pixels, its bytes, the designed plane (0: G, 1: R', 2: B'), its
    residuals, design letter, depth and prob_bits"""
    rs = np.random.RandomState(20250)
    n, out = 65536, {}

    def add8(name, design, pb, res, w=256, h=256, others=(9, 15)):
        px, res = tile8(res, w, h)
        out[name] = _case(name, design, 8, pb, px, res, (pb,) + tuple(others), 0)

    def add9(name, design, pb, res, plane=1, w=256, h=256, others=(8, 12)):
        px, res = tile9(res, w, h, plane)
        pbs = _other((others[0], others[1], others[1]), plane, pb)
        out[name] = _case(name, design, 9, pb, px, res, pbs, plane)

    grey = np.full((256, 256, 3), 128, np.uint8)
    out["a"] = _case("a", "a", 8, 8, grey, np.full(n, 128, np.uint16), (8, 9, 15), 0)
    for pb, oth in ((15, (10, 13)), (8, (9, 9)), (10, (15, 11)), (13, (12, 14))):
        add8("b8_%d" % pb, "b", pb, d_two(n, 128, 77), others=oth)
    add8("c8", "c", 15, d_burst(n, 256, 255, rs))
    add8("d8", "d", 15, d_burst(n, 256, 0, rs), others=(14, 10))
    add8("e8", "e", 15, d_equal(n, 256, rs))
    for pb in (9, 11, 12, 14):
        add8("g8_%d" % pb, "g", pb, d_geo(n, 128, 0.3, min(96, 1 << (pb - 4)), rs), others=(pb, 15))
    for pb, oth in ((15, (9, 10)), (9, (15, 9)), (11, (8, 13)), (14, (13, 11))):
        add9("b9_%d" % pb, "b", pb, d_two(n, 256, 300), plane=1 + pb % 2, others=oth)
    add9("burst9", "cd", 15, d_burst(n, 512, 256, rs), plane=2, others=(11, 9))   # both ends of the range
    add9("e9", "e", 15, d_equal(n, 512, rs), others=(15, 14))
    add9("f", "f", 15, d_full(n, rs), plane=2, others=(14, 15))
    for pb in (10, 12, 13):
        add9("g9_%d" % pb, "g", pb, d_geo(n, 256, 0.3, min(96, 1 << (pb - 4)), rs), plane=1 + pb % 2,
             others=(pb - 1, pb))
    # 300 x 300 tiles (flat layout, 90000 symbols: a last 1024-symbol segment of 912)
    m = 90000
    add8("c8_300", "c", 15, d_burst(m, 256, 255, rs, at=86 * 1024 + 800), w=300, h=300)
    add9("f_300", "f", 15, d_full(m, rs), plane=2, w=300, h=300, others=(13, 15))
    # LZ tiles: compacted planes below 1024 symbols and between 1024 and 16384
    for name, periods, pbs in (("lz_small", [3] * 250 + [4] * 6, (12, 13, 11)),
                               ("lz_mid", [37] * 253 + [38] * 3, (13, 11, 14))):
        px = _lz_tile(rs, periods)
        out[name] = _case(name, "lz", 8, pbs[0], px, None, pbs, None, lz=6)
    return out


FILES = {
    "F0": (1024, 512, ["a", "b8_15", "c8", "d8", "b9_9", "g9_10", "lz_small", "b9_15"]),
    "F1": (1024, 512, ["e8", "b8_8", "g8_9", "b8_10", "b9_11", "g9_12", "lz_mid", "burst9"]),
    "F2": (1024, 512, ["g8_11", "g8_12", "b8_13", "g8_14", "e9", "f", "g9_13", "b9_14"]),
    "F3": (600, 300, ["c8_300", "f_300"]),
}
# one window per file that crosses a tile edge in both directions
WINDOWS = {"F0": (200, 200, 120, 100), "F1": (700, 180, 200, 150), "F2": (450, 230, 130, 60),
           "F3": (250, 100, 100, 150)}


def file_prefix(W, H, sizes):
    """the tiled container's header and size table (what tiles_of reads back)"""
    return (bytes([153, 72, 79, 72, 2, 8]) + dr.wr_varint(W - 1) + dr.wr_varint(H - 1) +
            bytes([W // 256 - 1, H // 256 - 1]) + b"".join(dr.wr_varint(s) for s in sizes[:-1]))


@functools.lru_cache(maxsize=None)
def files():
    """name -> (file bytes, image, [(case name, tile offset in the file)])"""
    cs, out = cases(), {}
    for name, (W, H, names) in FILES.items():
        rects = dr.tile_rects(W, H)
        assert len(rects) == len(names)
        img = np.zeros((H, W, 3), np.uint8)
        tiles = []
        for (x0, y0, w, h), cn in zip(rects, names):
            assert cs[cn]["px"].shape == (h, w, 3)
            img[y0:y0 + h, x0:x0 + w] = cs[cn]["px"]
            tiles.append(cs[cn]["tile"])
        data = file_prefix(W, H, [len(t) for t in tiles]) + b"".join(tiles)
        offs, p = [], len(data) - sum(len(t) for t in tiles)
        for cn, t in zip(names, tiles):
            offs.append((cn, p))
            p += len(t)
        out[name] = (data, img, offs)
    return out


def stream_ends(parsed, tile_len):
    """byte offsets in the tile at which its three residual streams end (1x1 layers: 5 header bytes)"""
    e2 = tile_len
    e1 = e2 - 5 - len(parsed["layers"][2]["stream"])
    e0 = e1 - 5 - len(parsed["layers"][1]["stream"])
    return [e0, e1, e2]
