"""Planes built to reach a named decision of the -s1..-s4 predictor search and prob_bits ladder
(layer_encode.hpp:124-398; k_search.hip: k_search, k_search_walk_multi, k_prune_s, k_choose_s) -- the
third member of the family after tests/designed_streams.py and tests/designed_lz.py.  Pure numpy,
seeded.  What a plane is for is never taken on trust: tests/test_designed_search.py asserts every
claim below against the oracle's report (oracle.layer_report, the code or_layer_encode itself runs)
before a GPU test uses the plane.

* planted: per 40-px cell one predictor e of the sixteen (cells cycle through them); a pixel is
  p_e(L, T, TL, TR) plus noise, so every predictor is often the first of least error, ties between
  the two smallest errors abound (what cell_cost_multi's second-smallest key decides) and the
  search picks many different masks;
* ties: flat, row-constant and column-constant planes, where most cells' mask costs tie exactly
  at the minimum and `<` must keep the first;
* wrap: values at both ends of the range (the (T + L - TL) & 0xffff term, the residual wrap);
* ladder: one plane per outcome of the prob_bits ladder.

images() wraps planes into RGB tiles: G is an 8-bit design, R is chosen so that R - G + 256 is a
9-bit design, B is synth_rgb(noise=40)'s repeat-free blue, so no LZ match removes a design pixel and
a tile has more than 256 colours."""
import functools

import numpy as np

MASKS = [0x0001, 0x0002, 0x0020, 0x0010, 0xffbf, 0x0003, 0xfffd, 0xfffb, 0xfff7, 0xffef, 0xffdf, 0xff7f, 0xfdff,
         0xffff]                                              # layer_encode.hpp:159-175
NPRED = {1: 5, 2: 10, 3: 14, 4: 14}
SPEEDS = (1, 2, 3, 4)


def _orc():
    import oracle
    return oracle


# ------------------------------------------------------------------ the sixteen predictions, vectorised

def _midp(a, b):
    d = b - a
    return a + np.where(d >= 0, d // 2, -((-d) // 2))          # C division truncates


def preds(L, T, TL, TR):
    """prediction.hpp:190-207 on int64 arrays -> [16, n] (the whole-plane variant: paeth(L, TL, T))"""
    g = (T + L - TL) & 0xffff
    med = np.maximum(np.minimum(T, L), np.minimum(np.maximum(T, L), g))
    p = L + TL - T
    a, b, c = np.abs(L - p), np.abs(TL - p), np.abs(T - p)
    paeth = np.where(a < b, np.where(a < c, L, T), np.where(b < c, TL, T))
    return np.stack([L, T, TL, TR, med, _midp(L, T), _midp(L, TL), _midp(TL, T), _midp(T, TR), paeth,
                     (2 * L + TL) // 3, (L + 2 * TL) // 3, (2 * TL + T) // 3, (TL + 2 * T) // 3, (2 * T + TR) // 3,
                     (T + 2 * TR) // 3])


def planted(w, h, depth, seed, shift=0, lo=None, hi=None):
    """cell i of the 40-px grid plants predictor (i + shift) % 16: a pixel is that prediction of its
    neighbours, +-1..6 with probability 0.15, a uniform value with probability 0.02; the first row
    and column are uniform.  Values stay in [lo, hi] (clipped).  Pixels x + 2y = k depend on smaller
    k only, so a wavefront is one numpy step."""
    rs = np.random.RandomState(seed)
    c = 1 << depth
    lo = 0 if lo is None else lo
    hi = c - 1 if hi is None else hi
    xt, yt = (w + 39) // 40, (h + 39) // 40
    tw, th = (w + xt - 1) // xt, (h + yt - 1) // yt
    uni = rs.randint(lo, hi + 1, (h, w)).astype(np.int64)
    step = rs.randint(1, 7, (h, w)) * rs.choice([-1, 1], (h, w))
    u = rs.rand(h, w)
    d = uni.copy()
    yy, xx = np.mgrid[0:h, 0:w]
    e_of = ((yy // th) * xt + xx // tw + shift) % 16
    for k in range(3, w + 2 * h):
        y = np.arange(max(1, (k - w + 2) // 2), min(h - 1, (k - 1) // 2) + 1)
        x = k - 2 * y
        if not y.size:
            continue
        xr = np.minimum(x + 1, w - 1)
        p = preds(d[y, x - 1], d[y - 1, x], d[y - 1, x - 1], d[y - 1, xr])
        v = p[e_of[y, x], np.arange(y.size)]
        uu = u[y, x]
        v = np.where(uu < 0.15, v + step[y, x], v)
        v = np.where(uu > 0.98, uni[y, x], v)
        d[y, x] = np.clip(v, lo, hi)
    return d.astype(np.uint16)


def smooth(w, h, depth, seed, noise):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = (x * rs.randint(1, 5) + y * rs.randint(1, 5)) // 3 + rs.randint(-noise, noise + 1, (h, w))
    return (v % (1 << depth)).astype(np.uint16)


def geometric(w, h, seed, p):
    rs = np.random.RandomState(seed)
    return (128 + (rs.geometric(p, (h, w)) - 1) * rs.choice([-1, 1], (h, w))).clip(0, 255).astype(np.uint16)


def outliers(w, h, seed, base, frac, depth=8):
    """`base` (a plane or a value) with a fraction frac of uniform values"""
    rs = np.random.RandomState(seed)
    d = np.broadcast_to(np.asarray(base, np.uint16), (h, w)).copy()
    m = rs.rand(h, w) < frac
    d[m] = rs.randint(0, 1 << depth, int(m.sum()))
    return d


def checker(w, h, block, a=100, b=101):
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x // block + y // block) & 1, b, a).astype(np.uint16)


# ------------------------------------------------------------------ the planes

class Plane:
    def __init__(self, name, group, d, depth=8, nuke=None, want=None):
        self.name, self.group, self.d, self.depth, self.nuke, self.want = name, group, d, depth, nuke, want
        self.h, self.w = d.shape
        assert int(d.max()) < 1 << depth

    @property
    def cells(self):
        return ((self.w + 39) // 40) * ((self.h + 39) // 40)


# ladder outcomes (the report's view): name -> what tests/test_designed_search.py asserts at every speed
# (a dict: at those speeds)
#   ("med",)            the MED stream wins whole;   ("win", pb)  the trial at pb wins;
#   ("stale",)          the 16/15 pair's smaller size cuts the (valid) MED stream (Q14);
#   ("equal",)          t1 == t2 and every size is the stored size;   ("up", pb)  16 < 15, pb wins;
#   ("up-stale",)       16 < 15 and 16's size cuts the MED stream
@functools.lru_cache(maxsize=None)
def planes():
    out = {}

    def add(*a, **k):
        p = Plane(*a, **k)
        assert p.name not in out
        out[p.name] = p

    # 256 wide: cells of 37 with a cut last column (34); 300 x 260: k_search's w > 256 row loop and a
    # tile beyond the posting lists; 100 x 41: cells of 34 x 21, a cut last column (32) and row (20)
    add("planted256", "planted", planted(256, 256, 8, 11))
    add("planted300", "planted", planted(300, 260, 9, 12, shift=5, lo=1), depth=9)   # R - G + 256 is never 0
    add("planted100", "planted", planted(100, 41, 8, 13, shift=9))
    add("planted256b", "planted", planted(256, 256, 8, 14, shift=7))
    add("flat", "ties", np.full((256, 256), 77, np.uint16))
    y, x = np.mgrid[0:256, 0:256]
    add("rowconst", "ties", ((7 * y) % 256).astype(np.uint16))
    add("colconst", "ties", ((5 * x) % 256).astype(np.uint16))
    add("smooth256", "near", smooth(256, 256, 8, 21, 2))
    # both ends of the range: T + L - TL leaves [0, 2^depth) in both directions, residuals wrap
    # (patches of 23 x 17 of low and of high values, so both happen at patch edges)
    add("wrap8", "wrap", np.where((x // 23 + y // 17) & 1, planted(256, 256, 8, 32, lo=0, hi=6),
                                  planted(256, 256, 8, 33, lo=249, hi=255)).astype(np.uint16), want={2: ("up-stale",)})
    y9, x9 = np.mgrid[0:260, 0:300]
    add("wrap9", "wrap", np.where((x9 // 23 + y9 // 17) & 1, planted(300, 260, 9, 35, lo=1, hi=7),
                                  planted(300, 260, 9, 36, lo=505, hi=511)).astype(np.uint16), depth=9)
    add("lad_med", "ladder", checker(100, 41, 1), want=("med",))
    add("lad_14", "ladder", geometric(256, 256, 121, 0.3), want=("win", 14))
    add("lad_14tie12", "ladder", geometric(200, 200, 115, 0.5), want={1: ("win", 14)})   # 14 ties with 12 at -s1
    add("lad_13", "ladder", geometric(160, 160, 112, 0.1), want=("win", 13))
    add("lad_12", "ladder", geometric(100, 41, 100, 0.5), want=("win", 12))
    add("lad_stale15", "ladder", outliers(256, 256, 41, 100, 0.002), want=("stale",))
    add("lad_onebyte", "ladder", checker(300, 260, 2), want=("win", 13))
    add("lad_equal", "ladder", np.random.RandomState(42).randint(0, 256, (41, 100)).astype(np.uint16), want=("equal",))
    add("lad_up511", "ladder", outliers(511, 511, 43, 100 + (np.random.RandomState(44).rand(511, 511) < 0.5), 0.001),
        want=("up", 17))
    rs = np.random.RandomState(45)
    add("lad_nuke90", "ladder", geometric(256, 256, 46, 0.3), nuke=(rs.rand(256, 256) < 0.93).astype(np.uint8), want=None)
    add("lad_nukeall", "ladder", geometric(100, 41, 47, 0.3), nuke=np.ones((41, 100), np.uint8), want=None)
    return out


@functools.lru_cache(maxsize=None)
def report(name, speed):
    p = planes()[name]
    return _orc().layer_report(p.d, p.depth, speed, p.nuke)


@functools.lru_cache(maxsize=None)
def pixels(name):
    p = planes()[name]
    return _orc().pixel_report(p.d, p.depth)


def warm(fn, args):
    from concurrent.futures import ThreadPoolExecutor
    import os
    planes(), images()                                        # built once, not once per thread
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as ex:
        return list(ex.map(lambda a: fn(*a), args))


def outcome(r):
    """the ladder outcome of a report, in the vocabulary of Plane.want"""
    if r["error"]:
        return ("error", r["error"])
    if r["branch"] == 0:
        return ("none",)
    s = r["size"]
    if r["branch"] > 0:
        return ("up", r["winner"]) if r["winner"] > 0 else ("up-stale",) if r["stale"] else ("up-med",)
    if r["stale"]:
        return ("stale",)
    if r["winner"] > 0:
        return ("win", r["winner"])
    if s[16] == s[15] and len(set(s.values())) == 1 and s[15] == r["med_size"]:
        return ("equal",)
    return ("med",)


def tied_cells(r, p=-1):
    """cells of pass p whose least cost is reached by more than one mask"""
    c = r["cost"][p][:, :r["npred"]]
    return int(((c == c.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())


def near_ties(r, rel=1e-9):
    """(pass, cell) whose two best costs differ, by less than rel relative"""
    out = []
    for p in range(r["npass"]):
        c = np.sort(r["cost"][p][:, :r["npred"]], axis=1)
        gap = c[:, 1] - c[:, 0]
        for cell in np.flatnonzero((gap > 0) & (gap < rel * np.abs(c[:, 0]))):
            out.append((p, int(cell)))
    return out


# ------------------------------------------------------------------ images

def _blue(w, h, seed, ch=2):
    from hoh_ans.synth import synth_rgb
    return synth_rgb(w, h, seed, 40)[:, :, ch]


def windows_distinct(px):
    """every window of four consecutive pixels (tile raster order) occurs once: no LZ match of the
    shortest length kept (4) exists at any back distance, so no pixel is ever removed"""
    flat = np.ascontiguousarray(px, np.uint8).reshape(-1, 3)
    win = np.lib.stride_tricks.sliding_window_view(flat, (4, 3)).reshape(-1, 12)
    keys = np.ascontiguousarray(win).view(np.dtype((np.void, 12))).reshape(-1)
    return np.unique(keys).size == keys.size


def wrap_rgb(g8, r9, seed):
    """G = g8 (or, when None, the middle of the G that keeps R in 0..255); R so that R - G + 256 = r9
    (clipped where g8 leaves no such R; None: synth_rgb's red)"""
    ref = g8 if g8 is not None else r9
    h, w = ref.shape
    if g8 is None:
        g = (511 - r9.astype(np.int64)) // 2
    else:
        g = g8.astype(np.int64)
    r = _blue(w, h, seed, 0) if r9 is None else np.clip(r9.astype(np.int64) - 256 + g, 0, 255)
    return np.stack([r, g, _blue(w, h, seed)], -1).astype(np.uint8)


def image_planes(rgb):
    """the planes the encoder searches in a tile: 0 G, 1 R', 2 B', 4 R, 5 B (3, the indexed plane,
    only in palette tiles: palette_plane)"""
    rgb = rgb.astype(np.int64)
    R, G, B = rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]
    return {0: (G.astype(np.uint16), 8), 1: ((R - G + 256).astype(np.uint16), 9), 2: ((B - G + 256).astype(np.uint16), 9),
            4: (R.astype(np.uint16), 8), 5: (B.astype(np.uint16), 8)}


def palette_plane(rgb):
    """choh.cpp:62-88: indices in first-seen order"""
    px = rgb.reshape(-1, 3).astype(np.uint32)
    key = px[:, 0] | px[:, 1] << 8 | px[:, 2] << 16
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.argsort(np.argsort(first))
    return rank[inv].reshape(rgb.shape[:2]).astype(np.uint16)


def tiles_of(rgb):
    """[(x0, y0, w, h)] of choh.cpp:454-476; an untiled image is its own tile"""
    H, W, _ = rgb.shape
    if not ((W >= 512 or H >= 512) and W >= 256 and H >= 256):
        return [(0, 0, W, H)]
    xt, yt = W // 256, H // 256
    tw, th = (W + xt - 1) // xt, (H + yt - 1) // yt
    return [(x * tw, y * th, min(tw, W - x * tw), min(th, H - y * th)) for y in range(yt) for x in range(xt)]


@functools.lru_cache(maxsize=None)
def images():
    """name -> (H, W, 3) uint8.  Untiled images (at most 511 x 511) are single tiles: the plain choh
    writes their header only, OPT_SMALL_IMAGES the tile too."""
    P = planes()
    out = {}
    for name in ("planted256", "planted256b", "flat", "rowconst", "colconst", "wrap8", "lad_14", "lad_stale15",
                 "lad_13", "lad_onebyte", "lad_med", "lad_12", "lad_up511"):
        out[name] = wrap_rgb(P[name].d, None, 50 + len(out))
    for name in ("planted300", "wrap9"):
        out[name] = wrap_rgb(None, P[name].d, 50 + len(out))
    out["lad_equal"] = wrap_rgb(P["lad_equal"].d, None, 71)
    # both designed: G planted, R' planted around 256 (the G range leaves room)
    out["planted_both"] = wrap_rgb(planted(256, 256, 8, 15, lo=64, hi=191), planted(256, 256, 9, 16, shift=3, lo=192, hi=320), 70)
    # six tiles, four distinct tile pixel counts: 257 x 258, 256 x 258, 257 x 257, 256 x 257
    big = np.zeros((515, 770, 3), np.uint8)
    for k, (x0, y0, w, h) in enumerate(tiles_of(big)):
        big[y0:y0 + h, x0:x0 + w] = wrap_rgb(planted(w, h, 8, 80 + k, shift=k), None, 90 + k) if k % 2 == 0 else \
            wrap_rgb(None, planted(w, h, 9, 80 + k, shift=k, lo=1), 90 + k)
    out["planted770"] = big
    # a palette tile (<= 256 colours): plane 3, the indexed plane, is searched too
    rs = np.random.RandomState(61)
    pal = rs.randint(0, 256, (200, 3)).astype(np.uint8)
    out["palette256"] = pal[planted(256, 256, 8, 62, lo=0, hi=199)]
    return out


# ------------------------------------------------------------------ the oracle's answers for the images

IMAGE_NAMES = ("planted256", "planted256b", "lad_med", "lad_12", "lad_13", "lad_equal", "flat", "rowconst", "colconst", "wrap8", "lad_14", "lad_stale15", "lad_onebyte",
               "lad_up511", "planted300", "wrap9", "planted_both", "planted770", "palette256")
LZ_DIST = {1: 10, 2: 11, 3: 12, 4: 14}


def header(W, H):
    def vi(v):
        return bytes([v]) if v < 128 else bytes([(v >> 7) + 128, v % 128])
    return bytes([153, 72, 79, 72, 2, 8]) + vi(W - 1) + vi(H - 1)


@functools.lru_cache(maxsize=None)
def image_file(name, speed):
    """-> (the plain file, its printed size, the file with the tile: OPT_SMALL_IMAGES for an untiled
    image) or the oracle's error.  An untiled image's plain file is its header."""
    orc, img = _orc(), images()[name]
    H, W, _ = img.shape
    try:
        if len(tiles_of(img)) > 1:
            f, printed = orc.choh(img, speed)
            return f, printed, f
        t = orc.encode_tile(img, speed)
        return header(W, H), len(header(W, H)) + len(t), header(W, H) + t
    except orc.OracleError as e:
        return e


def tile_pixels(name, k):
    x0, y0, w, h = tiles_of(images()[name])[k]
    return np.ascontiguousarray(images()[name][y0:y0 + h, x0:x0 + w])


@functools.lru_cache(maxsize=None)
def tile_nuke(name, k, speed):
    """the positions LZ copies take out of the tile's planes: none where every 4-pixel window is
    distinct (tests/test_designed_search.py), else the oracle's find_lz at the speed's distance"""
    px = tile_pixels(name, k)
    if windows_distinct(px):
        return None
    import designed_lz as DL
    orc = _orc()
    cc = orc.lib().or_count_colours(px.ctypes.data_as(orc.u8p), px.size)
    h, w, _ = px.shape
    return DL.find_lz(orc.lib().or_find_lz_rgb, px, w, h, LZ_DIST[speed], DL.threshold(cc) - 4)[1].reshape(h, w)


def searched_planes(name, k, speed):
    """plane slots the encoder searches in the tile: 0 G, 1 R', 2 B', 3 indexed (at most 256 colours),
    4 R and 5 B (-s3 / -s4)"""
    px = tile_pixels(name, k)
    orc = _orc()
    pal = orc.lib().or_count_colours(px.ctypes.data_as(orc.u8p), px.size) != -1
    return [0, 1, 2] + ([3] if pal else []) + ([4, 5] if speed >= 3 else [])


@functools.lru_cache(maxsize=None)
def _tile_report(name, k, plane, speed):
    px = tile_pixels(name, k)
    d, depth = (palette_plane(px), 8) if plane == 3 else image_planes(px)[plane]
    return _orc().layer_report(d, depth, speed, tile_nuke(name, k, speed))


def tile_report(name, k, plane, speed):
    """the oracle's report for one searched plane of an image's tile (cruncher 3 and 4 differ in the
    LZ window alone)"""
    if speed == 4 and tile_nuke(name, k, 4) is None:
        speed = 3
    return _tile_report(name, k, plane, speed)


def report_jobs(names=IMAGE_NAMES):
    return [(n, k, p, sp) for n in names for k in range(len(tiles_of(images()[n]))) for sp in SPEEDS
            for p in searched_planes(n, k, sp)]


def decodable_choice(r):
    """HOH_OPT_DECODABLE's ladder on a report: 16..19 if s(16) < s(15) else 15..12, the first of
    strictly smallest size"""
    s = r["size"]
    cand = [16, 17, 18, 19] if s[16] < s[15] else [15, 14, 13, 12]
    best = cand[0]
    for pb in cand[1:]:
        if s[pb] < s[best]:
            best = pb
    return best


def seek(limit=100):
    """the outcomes looked for and not required: prob_bits 18 / 19 winning, the invalid layer.  Seeded,
    at most `limit` planes; prints what it finds (python tests/designed_search.py)."""
    found = {}
    for k in range(limit):
        rs = np.random.RandomState(1000 + k)
        side = int(rs.choice([256, 400, 511]))
        nlev = int(rs.choice([1, 2, 3]))
        base = 100 + (rs.rand(side, side) * nlev).astype(np.int64) if nlev > 1 else 100
        d = outliers(side, side, 2000 + k, base, float(rs.choice([0.0, 0.0002, 0.001, 0.005])))
        nuke = (rs.rand(side, side) < 0.5).astype(np.uint8) if k % 5 == 4 else None
        o = outcome(_orc().layer_report(d, 8, 1, nuke))
        found.setdefault(o, []).append(k)
    for o, ks in sorted(found.items()):
        print(o, len(ks), ks[:6])
    return found


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hoh-ans_amd"))
    seek()
