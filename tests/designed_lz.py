"""Single tiles whose LZ matches are chosen, not found in an image: the encoder-side counterpart of
tests/designed_streams.py.  Every tile is synth_rgb(noise=40) -- repeat-free at every seek window --
with copies pasted in tile raster order, and comes with the matches lz.hpp:6-170's greedy search
must report at each seek distance (6, 10, 11, 12, 14 for -s0..-s4, choh.cpp:125-137).

A paste(p, L, b) copies [p - b, p - b + L) to [p, p + L).  Two rules keep a paste's match what it
claims to be:

* the pristine-source rule: the source is base noise that nothing has been pasted to and that no
  other paste uses, so the same content exists at no nearer back (Tile.used enforces it);
* fences: the pixels just before and just after the source and the copy take colours that occur
  nowhere else in the tile, so no equal neighbour moves the match's start or end.

expected(tile, dist) walks the designed spans only, with the designed backs only, by the
reference's rule -- the window's backs nearest first and strictly longer, a stop at 259, then
(distance > 8, longest < 259) the whole-row backs up to 65536, strictly longer -- comparing the
tile's real pixels.  A tile's match list must equal it: whatever is pasted from beyond the window
by a back that is no whole number of rows must not appear.  (The bonus tiles, random pixels of a
few colours, hold chance matches besides: their lists contain the claims.)

The boundaries come from k_lzscan's launch (k_search.hip, encode_speed_s: rp = min(ring, limit +
324 rounded up), reach = rp - 324): 1024-position rings at -s1/-s2 serve backs <= 700, 512-position
rings at -s3/-s4 backs <= 188; longer backs compare pixel words from memory.  Segment starts of
the four-wave walk of a 65,536-position tile: 16384, 32768, 49152."""
import functools
import os

import numpy as np

DISTANCES = (6, 10, 11, 12, 14)
SPEED_DIST = {0: 6, 1: 10, 2: 11, 3: 12, 4: 14}
SHAPES = ((256, 256), (300, 260))
RING_REACH = (188, 700)                       # k_search.hip encode_speed_s: 512 - 324, 1024 - 324
SEG_STARTS = (16384, 32768, 49152)
SWEEP_BACKS = (1, 2, 3, 4, 63, 64, 65, 187, 188, 189, 190, 255, 256, 257, 699, 700, 701, 702, 1023, 1024, 1025,
               2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385)
SWEEP_LENGTHS = (4, 5, 16, 17, 32, 33, 258, 259, 260, 263, 600)
RUN_LENGTHS = (3, 4, 5, 254, 255, 256, 258, 259, 260, 509, 510, 511, 514, 700)
BONUS_COLOURS = (4, 5, 8, 9, 16, 17, 32, 33)
CAP = 259
# rowperiod's dense posting group.  Twelve positions apart: closer, rowperiod70's -s0 file takes a
# raw frequency table whose 8-bit fields overflow and no decoder reads it back
DENSE_AT, DENSE_STEP, DENSE_N = 300, 12, 150


def _orc():
    import oracle
    return oracle


def threshold(colours):
    """shortest match kept (choh.cpp:139-154: 4 + the colour-count bonus); colours -1: more than 256"""
    if colours == -1 or colours > 32:
        return 4
    return 36 if colours <= 4 else 24 if colours <= 8 else 14 if colours <= 16 else 6


def pack(px):
    px = np.asarray(px).reshape(-1, 3).astype(np.uint32)
    return px[:, 0] | px[:, 1] << 8 | px[:, 2] << 16


def paste(tile, p, L, b):
    """an LZ repeat of length L at back distance b starting at tile raster position p"""
    for i in range(L):
        tile[p + i] = tile[p + i - b]


# ------------------------------------------------------------------ a tile under construction

class Tile:
    def __init__(self, name, w, h, seed, px=None, fence_with=None):
        from hoh_ans.synth import synth_rgb
        self.name, self.w, self.h, self.n = name, w, h, w * h
        self.px = (synth_rgb(w, h, seed, 40) if px is None else px).reshape(-1, 3).copy()
        self.used = np.zeros(self.n, bool)
        self.spans, self.pastes, self.backs = [], [], set()
        self.exact = True                     # the match list equals expected(); else it contains the claims
        self._rs = np.random.RandomState(seed)
        self._seen = set(pack(self.px).tolist())
        self._fence_with = fence_with

    @property
    def shape(self):
        return "%dx%d" % (self.w, self.h)

    def image(self):
        return self.px.reshape(self.h, self.w, 3)

    def fresh(self):
        while True:
            c = self._rs.randint(0, 256, 3)
            k = int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16
            if k not in self._seen:
                self._seen.add(k)
                return c

    def fence(self, q, other=()):
        """position q gets a colour found nowhere else (a palette tile: one that differs from the
        pixels at `other`)"""
        if not 0 <= q < self.n:
            return
        if self._fence_with is None:
            self.px[q] = self.fresh()
        elif other:
            ban = {int(pack(self.px[o])[0]) for o in other if 0 <= o < self.n}
            self.px[q] = next(c for c in self._fence_with if int(pack(c)[0]) not in ban)
        self.used[q] = True

    def free(self, lo, hi):
        return lo >= 0 and hi <= self.n and not self.used[max(lo, 0):hi].any()

    def take(self, lo, hi):
        assert self.free(max(lo, 0), min(hi, self.n)), (self.name, lo, hi)
        self.used[max(lo, 0):min(hi, self.n)] = True

    def copy(self, p, L, b, claim=True, shared=False):
        """paste with fences; the source [p - b, p - b + L) must be pristine (shared: it is another
        copy's source or a copy of one -- the caller says what follows from that)"""
        assert 1 <= b <= p and p + L <= self.n, (self.name, p, L, b)
        if b <= L + 1:                                        # overlapping: one region, period b
            self.take(p - b - 1, p + L + 1)
            self.fence(p - b - 1)
        else:
            self.take(p - 1, p + L + 1)
            if not shared:
                self.take(p - b - 1, p - b + L + 1)
                self.fence(p - b - 1)
                self.fence(p - b + L)
            self.fence(p - 1, (p - 1 - b,))
        paste(self.px, p, L, b)
        self.fence(p + L, (p + L - b,))
        self.spans.append((p, L))
        self.backs.add(b)
        if claim:
            self.pastes.append((p, L, b))
        return p

    def place(self, L, b, start=0, step=1):
        """the first p >= start at which copy(p, L, b) finds room"""
        p = max(start, b + 1)
        while True:
            assert p + L + 1 <= self.n, (self.name, L, b)
            if b <= L + 1:
                ok = self.free(p - b - 1, p + L + 1)
            else:
                ok = self.free(p - 1, p + L + 1) and self.free(p - b - 1, p - b + L + 1)
            if ok:
                return self.copy(p, L, b)
            p += step

    def chain(self, p, alts):
        """the content at p also stands at every p - b of alts = [(b, L), ...], equal for exactly L
        pixels; the farthest holds the longest.  The nearer sources are copies of the farthest (and
        spans of their own: they match it where it is in reach)."""
        alts = sorted(alts, reverse=True)
        b0, L0 = alts[0]
        assert all(L <= L0 for _, L in alts)
        while not (self.free(p - 1, p + L0 + 1) and all(self.free(p - b - 1, p - b + L + 1) for b, L in alts)):
            p += 1
        self.take(p - b0 - 1, p - b0 + L0 + 1)
        self.fence(p - b0 - 1)
        self.fence(p - b0 + L0)
        for b, L in alts[1:]:
            self.copy(p - b, L, b0 - b, claim=False, shared=True)
            for b2, L2 in alts[1:]:
                if b2 > b:
                    self.backs.add(b2 - b)
        self.copy(p, L0, b0, claim=False, shared=True)
        self.backs.update(b for b, _ in alts)
        return p


# ------------------------------------------------------------------ the reference's rule on designed spans

def _common(key, pos, backs):
    """equal pixels from pos against pos - b for every b, at most 259"""
    m = min(CAP, key.size - pos)
    eq = key[(pos - backs)[:, None] + np.arange(m)[None, :]] == key[None, pos:pos + m]
    return np.where(eq.all(axis=1), m, np.argmin(eq, axis=1))


def greedy_at(key, pos, backs, w, dist):
    """(longest, back) at pos over the ascending candidate backs (lz.hpp:32-74)"""
    backs = np.asarray(backs, np.int64)
    longest, best = 0, -1
    hb = backs[backs <= min(1 << dist, pos)]
    if hb.size:
        L = _common(key, pos, hb)
        i = int(np.argmax(L))                                 # nearest of the longest (the first 259 stops it)
        longest, best = int(L[i]), int(hb[i])
    if longest < CAP and dist > 8:
        vb = backs[(backs % w == 0) & (backs <= min(65536, pos))]
        if vb.size:
            L = _common(key, pos, vb)
            i = int(np.argmax(L))
            if int(L[i]) > longest:
                longest, best = int(L[i]), int(vb[i])
    return longest, best


def expected(t, dist):
    """the matches (pos, len, back & 0xffff) of the designed spans (back 65536 is written as 0)"""
    key = pack(t.px)
    thr = threshold(t.colours)
    out, pos = [], 0
    for s, L in sorted(t.spans):
        pos = max(pos, s)
        while pos < s + L:
            cands = t.cands(key, pos) if hasattr(t, "cands") else np.array(sorted(b for b in t.backs if b <= pos))
            longest, best = greedy_at(key, pos, cands, t.w, dist) if len(cands) else (0, -1)
            if longest >= thr:
                out.append((pos, longest, best & 0xffff))
                pos += longest
            else:
                pos += 1
    return out


def visible(b, w, dist):
    """whether the reference's search at this seek distance tries back b at all"""
    return b <= 1 << dist or (dist > 8 and b % w == 0 and b <= 65536)


def claims(t, dist):
    """the single-source pastes as the issue states them: (p, min(L, 259), b) and its follow-ups where
    b is in reach at this distance (-> must), else the span no match may touch (-> never)"""
    must, never = [], []
    thr = threshold(t.colours)
    for p, L, b in t.pastes:
        if visible(b, t.w, dist):
            q = p
            while p + L - q >= thr:
                must.append((q, min(p + L - q, CAP), b & 0xffff))
                q += CAP
        else:
            never.append((p, L, b))
    return must, never


# ------------------------------------------------------------------ the oracle's answer

def find_lz(fn, px, w, h, dist, bonus):
    """(stream bytes, nuke map) of or_find_lz_rgb / ref_find_lz_rgb"""
    O = _orc()
    px = np.ascontiguousarray(px, np.uint8).reshape(-1)
    out = np.zeros(4 * O.lib().or_entropy_bound(w * h, 256, 10) + 64, np.uint8)
    nuke = np.zeros(w * h, np.uint8)
    r = fn(px.ctypes.data_as(O.u8p), px.size, w, h, out.ctypes.data_as(O.u8p), nuke.ctypes.data_as(O.u8p), dist, bonus)
    assert r > 0, r
    return out[:r].tobytes(), nuke


def parse_matches(data, dist):
    """the LZ streams (lz.hpp:76-142: future with its 255 escape, length - 4, backby, backby2) ->
    [(pos, len, back)]; back 65536 reads as 0"""
    O = _orc()
    assert data[0] == 0x03
    bp, streams = 1, []
    for _ in range(4 if dist > 8 else 3):
        s, bp = O.decode_entropy(data, bp)
        streams.append(s.astype(np.int64))
    assert bp == len(data)
    fut, ln, bb = streams[:3]
    back = bb + (256 * streams[3] if dist > 8 else 0)
    out, pos, m = [], 0, 0
    for v in fut.tolist():
        if v == 255:
            pos += 255
            continue
        pos += v
        out.append((pos, int(ln[m]) + 4, int(back[m])))
        pos += int(ln[m]) + 4
        m += 1
    assert m == ln.size == back.size
    return out


def ref_matches(tile, w, h, dist, bonus):
    return parse_matches(find_lz(_orc().lib().or_find_lz_rgb, tile, w, h, dist, bonus)[0], dist)


def encode_matches(matches, npix, dist):
    """parse_matches' inverse: find_lz's bytes for a match list"""
    fut, pos = [], 0
    for p, L, _ in matches:
        fut += [255] * ((p - pos) // 255) + [(p - pos) % 255]
        pos = p + L
    fut += [255] * ((npix - pos) // 255)
    streams = [fut, [L - 4 for _, L, _ in matches], [b % 256 for _, _, b in matches]]
    if dist > 8:
        streams.append([b // 256 % 256 for _, _, b in matches])
    return b"\x03" + b"".join(_orc().encode_entropy(np.array(s, np.uint16), 256, 10) for s in streams)


def oracle_matches(key, dist):
    """the oracle's match list for a design.  Where a stream's table cannot be read back (a raw
    table whose 8-bit fields a frequency of 256 or more overflows), the list is
    expected()'s once it codes to the oracle's very bytes."""
    data = oracle_lz(key, dist)[0]
    try:
        return parse_matches(data, dist)
    except _orc().OracleError as e:
        t = designs()[key]
        want = expected(t, dist)
        assert e.code == -5 and t.exact and encode_matches(want, t.n, dist) == data, (key, dist, e.code)
        return want


# the oracle takes seconds per tile at the long windows: every answer is computed once per process,
# several at a time (ctypes calls run without the interpreter lock), and shared by the tests

@functools.lru_cache(maxsize=None)
def oracle_lz(key, dist):
    """(stream bytes, nuke map) of the oracle's find_lz for design key = (name, shape)"""
    t = designs()[key]
    return find_lz(_orc().lib().or_find_lz_rgb, t.px, t.w, t.h, dist, threshold(t.colours) - 4)


@functools.lru_cache(maxsize=None)
def oracle_tile(key, speed):
    """the oracle's encode_tile bytes (an OracleError instance where the reference's are undefined)"""
    try:
        return _orc().encode_tile(designs()[key].image(), speed)
    except _orc().OracleError as e:
        return e


def warm(fn, args):
    """fn(*a) for every a of args on a few threads, for the caches above"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as ex:
        return list(ex.map(lambda a: fn(*a), args))


def lz_jobs():
    return [(k, SPEED_DIST[sp]) for k, t in designs().items() for sp in speeds_of(t)]


def tile_jobs():
    return [(k, sp) for k, t in designs().items() for sp in speeds_of(t)]


# ------------------------------------------------------------------ the designs

def d_sweep(w, h, seed, rot):
    t = Tile("sweep", w, h, seed)
    start = 300
    for i, b in enumerate(SWEEP_BACKS):
        L = SWEEP_LENGTHS[(i + rot) % len(SWEEP_LENGTHS)]
        start = t.place(L, b, start) + L + 40 + 13 * (i % 5)
    return t


def d_vertical(w, h, seed):
    """copies from exactly k rows up: k * w just inside each window, just beyond it, as far as fits
    (and, where rows are left, past 65536); twins at k * w +- 1 beyond every window; a horizontal
    source as long (it wins) and a pixel shorter (the vertical one wins)"""
    t = Tile("vertical", w, h, seed)
    ks = sorted({k for lim in (1024, 2048, 4096, 16384) for k in (lim // w, lim // w + 1) if 0 < k < h}
                | {min(h - 1, 65536 // w)} | ({65536 // w + 1} if 65536 // w + 1 < h else set()))
    far = max(k for k in ks if k * w <= 65536)
    x = 5
    for i, k in enumerate(ks[::-1]):                          # the farthest first: its rows are the scarce ones
        L = 300 if k == 16384 // w else 100 if k == far else (20, 41, 7)[i % 3]
        t.place(L, k * w, k * w + (3 if k >= far else x))
        x = (x + L + 37) % (w - 108)
    kt = 16384 // w + 1                                       # beyond every window
    for d, xx in ((-1, 30), (1, 90)):
        t.place(24, kt * w + d, (kt + 3) * w + xx)
    row = kt + 20
    t.tie_h = (t.chain(row * w + 20, [(kt * w, 30), (37, 30)]), 30, 37)
    t.tie_v = (t.chain(row * w + 120, [(kt * w, 31), (41, 30)]), 31, kt * w)
    return t


def d_tall(w, h, seed, ks):
    """narrow or tall single tiles: copies from the given numbers of rows up, twins one off"""
    t = Tile("vertical", w, h, seed)
    for i, (k, L) in enumerate(zip(ks, (12, 270, 40))):
        t.place(L, k * w, k * w + 3 + (w + 17 if i == 1 else 0))
    k = ks[0]
    for d in (-1, 1):
        t.place(16, k * w + d, k * w + 5 * w + (20 if d < 0 else 3 * w))
    return t


def d_ties(w, h, seed):
    t = Tile("ties", w, h, seed)
    t.cases = {}
    p = 3000
    for name, alts in (("near-64", [(60, 20), (25, 20)]), ("near-1024", [(900, 25), (300, 25)]),
                       ("near-16384", [(9000, 18), (5000, 18)]),
                       ("longer-64", [(62, 23), (26, 20)]), ("longer-1024", [(1000, 40), (250, 33)]),
                       ("longer-4096", [(3900, 12), (1500, 8)]),
                       ("cap-3", [(1000, 300), (650, 300), (310, 300)]), ("cap-2-far", [(15000, 259), (7000, 259)])):
        p = max(p, max(b for b, _ in alts) + 2000)
        p = t.chain(p, alts)
        t.cases[name] = (p, alts)
        p += max(L for _, L in alts) + 700
    return t


def d_runs(w, h, seed):
    """flat runs of one colour between noise, a second colour's runs interleaved; some runs start
    at a tile row start and at the row's last pixel.  Candidates: every earlier pixel of the colour."""
    t = Tile("runs", w, h, seed)
    A, B = t.fresh(), t.fresh()
    blens = (5, 40, 300, 12, 260, 4, 33)
    p, runs = 700, []
    for i, n in enumerate(RUN_LENGTHS):
        if i % 4 == 1:
            p = (p // w + 1) * w                              # a row start
        elif i % 4 == 3:
            p = (p // w + 1) * w + w - 1                      # the row's last pixel
        runs.append((p, n, A))
        p += n + 9 + 31 * (i % 3)
        if i % 2 == 0:
            m = blens[(i // 2) % len(blens)]
            runs.append((p, m, B))
            p += m + 23
    for s, n, c in runs:
        t.take(s - 1, s + n + 1)
        t.fence(s - 1)
        t.fence(s + n)
        t.px[s:s + n] = c
        t.spans.append((s, n))
    t.runs = runs
    t.cands = lambda key, pos: pos - np.flatnonzero(key[:pos] == key[pos])[::-1]
    return t


def d_stitch(seed):
    """256 x 256: at each segment start X a copy of 259 + 150 from X - 100 and a second source that
    joins inside its tail: the segment's own walk from X differs from the tile's up to X + 500"""
    t = Tile("stitch", 256, 256, seed)
    for X, b, b2 in zip(SEG_STARTS, (900, 3000, 9000), (650, 1500, 5 * 256)):
        # [X - 100, X + 309) from back b; [X + 200, X + 500) from back b2, whose source holds b's in its first 109
        t.take(X - 100 - b - 1, X + 309 - b + 1)
        t.fence(X - 100 - b - 1)
        t.fence(X + 309 - b)
        q2 = X + 200 - b2
        t.take(q2 - 1, q2 + 301)
        t.fence(q2 - 1)
        t.fence(q2 + 300)
        paste(t.px, q2, 109, b - b2)
        t.take(X - 101, X + 501)
        t.fence(X - 101)
        paste(t.px, X - 100, 300, b)
        paste(t.px, X + 200, 300, b2)
        t.fence(X + 500)
        t.spans += [(q2, 109), (X - 100, 600)]
        t.backs.update((b, b2, b - b2))
    return t


def d_stitch_edges(seed):
    """256 x 256: a copy that starts exactly on a segment start, one that ends exactly on one, and a
    capped one (263) from one"""
    t = Tile("stitch-edges", 256, 256, seed)
    t.copy(SEG_STARTS[0], 40, 500)
    t.copy(SEG_STARTS[1] - 40, 40, 2100)
    t.copy(SEG_STARTS[2], 263, 5000)
    return t


def d_gaps(w, h, seed):
    """matches separated by exactly 254, 255, 256, 509 and 510 unmatched positions, the first at
    position 255, the last ending on the tile's last pixel"""
    t = Tile("gaps", w, h, seed)
    p = 255
    for gap in (254, 255, 256, 509, 510, None):
        t.copy(p, 8, 100)
        if gap is not None:
            p += 8 + gap
    t.copy(t.n - 12, 12, 77)
    return t


def d_bonus(w, h, seed, ncol):
    """random pixels of ncol colours with one green; two far copies, one the threshold long and one
    a pixel shorter"""
    rs = np.random.RandomState(seed)
    rb = rs.permutation(65536)[:ncol]
    pal = np.stack([rb >> 8, np.full(ncol, 9), rb & 255], 1).astype(np.uint8)
    t = Tile("bonus%d" % ncol, w, h, seed, px=pal[rs.randint(0, ncol, w * h)], fence_with=pal)
    t.exact = False
    thr = threshold(ncol)
    t.copy(20000, thr, 900)
    t.short = (40000, thr - 1, 900)
    t.copy(*t.short, claim=False)
    return t


def d_rowperiod(seed, k):
    """256 x 256: every row repeats the one k rows up, so every position is a vertical candidate.
    Rows repeating k rows on put at most 256 / k equal windows into a posting group, so the first
    rows also hold one four-pixel window 150 times, twelve positions apart with nothing else equal
    around it: more than 64 entries of one group inside the shortest window (1024), each four
    long, so a walk from a later one takes several batches -- and every copy of these rows still
    finds the 259 from k rows up."""
    t = Tile("rowperiod%d" % k, 256, 256, seed)
    b = k * 256
    gram = [t.fresh() for _ in range(4)]
    for i in range(DENSE_N):
        q = DENSE_AT + DENSE_STEP * i
        t.px[q:q + 4] = gram
        for x in range(q + 4, q + DENSE_STEP):
            t.fence(x)
    t.spans.append((DENSE_AT, DENSE_STEP * DENSE_N))
    t.backs.update(DENSE_STEP * i for i in range(1, DENSE_N))
    t.used[:] = False
    t.take(0, t.n)
    paste(t.px, b, t.n - b, b)
    t.spans.append((b, t.n - b))
    t.backs.add(b)
    return t


def _finish(t):
    t.colours = _orc().lib().or_count_colours(t.px.ctypes.data_as(_orc().u8p), t.px.size)
    return t


@functools.lru_cache(maxsize=None)
def designs():
    """(name, shape) -> tile"""
    out = {}

    def add(t):
        out[(t.name, t.shape)] = _finish(t)

    for i, (w, h) in enumerate(SHAPES):
        add(d_sweep(w, h, 101 + i, 5 * i))
        add(d_vertical(w, h, 111 + i))
        add(d_ties(w, h, 121 + i))
        add(d_runs(w, h, 131 + i))
        add(d_gaps(w, h, 141 + i))
        for n in BONUS_COLOURS:
            add(d_bonus(w, h, 151 + i, n))
    add(d_tall(256, 300, 161, (256, 200, 299)))                 # 65536 back (written as 0 / 0); 299 rows: beyond it, never
    add(d_tall(64, 511, 162, (300, 257, 510)))
    add(d_tall(140, 400, 163, (300, 257, 399)))
    add(d_tall(300, 200, 164, (100, 60, 199)))                  # posting lists and wider than k_lzvert's 256
    add(d_stitch(171))
    add(d_stitch_edges(172))
    add(d_rowperiod(181, 9))
    add(d_rowperiod(182, 70))
    return out


def speeds_of(t):
    return (1, 4) if t.name.startswith("bonus") else (0, 1, 2, 3, 4)
