"""GPU: HOH_OPT_CHAIN_TABLES -- the prob_bits-15 encoder chain with its streams' hot windows in LDS
(k_rans_enc.hip, HOT) against the same chain gathering every entry from memory, and both against
the CPU oracle, byte for byte.  The window only decides where a table entry is read from, so every
setting must give the oracle's bytes; the cases are built so that hits, misses and both window
edges are really taken (asserted on the CPU from the histograms, not assumed)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

K = 32               # CHAIN_HOT_K (hoh_internal.h)
FAST_RANGE = 512     # HOH_FAST_RANGE
LENGTHS = (1, 31, 32, 33, 71, 4096 + 5, 65536)


@pytest.fixture(scope="module")
def hoh():
    import torch  # noqa: F401  (before the first context: torch brings its own HIP runtime)
    import hoh_ans
    return hoh_ans


@pytest.fixture(scope="module")
def ctxs(hoh):
    """one context per setting: auto, the LDS window pinned, the global gathers pinned"""
    c = {"auto": hoh.Context(0), "lds": hoh.Context(0), "global": hoh.Context(0)}
    c["auto"].set_option(hoh.OPT_CHAIN_TABLES, hoh.CHAIN_TABLES_AUTO)
    c["lds"].set_option(hoh.OPT_CHAIN_TABLES, hoh.CHAIN_TABLES_LDS)
    c["global"].set_option(hoh.OPT_CHAIN_TABLES, hoh.CHAIN_TABLES_GLOBAL)
    yield c
    for v in c.values():
        v.close()


def window(orc, sym, rng):
    """k_tables' choice restated: over the normalised frequencies, the lo in [0, 512 - K] of
    largest mass cum[min(lo + K, range)] - cum[min(lo, range)], ties to the lowest lo."""
    _, cum = orc.normalize_freqs(np.bincount(sym, minlength=rng).astype(np.uint32), 1 << 15)
    cum = cum.astype(np.int64)
    lo = np.arange(FAST_RANGE - K + 1)
    mass = cum[np.minimum(lo + K, rng)] - cum[np.minimum(lo, rng)]
    best = int(np.argmax(mass))                       # first maximum: the lowest lo
    return best, int(mass[best])


def span(sym):
    return int(sym.max()) - int(sym.min()) + 1


def check_all(hoh, orc, ctxs, sym, rng):
    want = orc.encode_entropy(sym, rng, 15)
    for name, ctx in ctxs.items():
        got = hoh.encode_entropy(sym, rng, 15, ctx=ctx)
        assert bytes(got) == bytes(want), "CHAIN_TABLES %s: range %d, n %d" % (name, rng, sym.size)


def edge_stream(rng, lo, n, seed):
    """Two heavy symbols at lo and lo + K - 1 (so the best window is [lo, lo + K) alone), light
    ones just outside it at lo - 1 and lo + K where the alphabet has them, a few in between; the
    four edge symbols are placed at both ends of the stream when it is long enough."""
    r = np.random.default_rng(seed)
    inside = [lo, lo + K - 1]
    outside = [s for s in (lo - 1, lo + K) if 0 <= s < rng]
    mid = [lo + 1, lo + K // 2, lo + K - 2]
    vals = np.array(inside + mid + outside)
    p = np.array([0.38, 0.38] + [0.06] * 3 + [0.03] * len(outside))
    sym = r.choice(vals, size=n, p=p / p.sum()).astype(np.uint16)
    edges = np.array(inside + outside, np.uint16)
    if n >= 2 * edges.size:
        sym[:edges.size] = edges
        sym[n - edges.size:] = edges[::-1]
    return sym, outside


# the window at the bottom (mode 0: no symbol below it), in the middle (all four edges), and
# clamped at the top of the alphabet (mode range - 1: no symbol above it)
@pytest.mark.parametrize("rng", [256, 512])
@pytest.mark.parametrize("place", ["bottom", "middle", "top"])
def test_window_edges(hoh, orc, ctxs, rng, place):
    lo = {"bottom": 0, "middle": 100, "top": rng - K}[place]
    for i, n in enumerate(LENGTHS):
        sym, outside = edge_stream(rng, lo, n, 100 * rng + i)
        if n >= 71:
            # the histogram really puts the window at lo, with symbols on both of its edges inside
            # and the neighbours outside: hits and misses are both taken, at d = 0, K - 1, -1, K
            assert window(orc, sym, rng)[0] == lo
            present = set(sym.tolist())
            assert {lo, lo + K - 1} <= present and set(outside) <= present and outside
        check_all(hoh, orc, ctxs, sym, rng)


@pytest.mark.parametrize("rng", [256, 512])
def test_all_hits_all_misses_two_peaks(hoh, orc, ctxs, rng):
    r = np.random.default_rng(rng)
    for n in (33, 4096 + 5, 65536):
        # <= K distinct consecutive symbols: one window holds every symbol
        hits = (40 + r.integers(0, K, n)).astype(np.uint16)
        assert span(hits) <= K
        lo, mass = window(orc, hits, rng)
        assert mass == 1 << 15 and lo <= int(hits.min()) and int(hits.max()) < lo + K
        check_all(hoh, orc, ctxs, hits, rng)
        # uniform over the alphabet: no window holds more than ~K / range of the symbols
        uni = r.integers(0, rng, n).astype(np.uint16)
        if n >= 4096:
            assert window(orc, uni, rng)[1] < (1 << 15) // 4 and span(uni) > K
        check_all(hoh, orc, ctxs, uni, rng)
        # two peaks more than K apart: whichever the window takes, the other always misses
        a, b = 20, 20 + 3 * K
        two = np.where(r.random(n) < 0.6, a + r.integers(0, 4, n), b + r.integers(0, 4, n)).astype(np.uint16)
        lo, mass = window(orc, two, rng)
        assert span(two) > K and mass < 1 << 15
        if n >= 4096:
            assert lo <= a + 3 < lo + K and not (lo <= b < lo + K)      # the heavier peak, whole
        check_all(hoh, orc, ctxs, two, rng)


@pytest.mark.parametrize("rng", [2, 16])
def test_range_below_window(hoh, orc, ctxs, rng):
    r = np.random.default_rng(rng)
    for n in LENGTHS:
        sym = np.minimum(r.geometric(0.4, n) - 1, rng - 1).astype(np.uint16)
        assert window(orc, sym, rng) == (0, 1 << 15)      # the whole alphabet, tie to lo = 0
        check_all(hoh, orc, ctxs, sym, rng)


def test_window_choice_read_back(orc):
    """hot_lo and the window's mass as k_tables stored them (the checking build's StreamInfo
    read-back: the words a size-only trial uses for its bounds) against the numpy restatement,
    ties included."""
    import torch  # noqa: F401
    from checklib import CheckLib
    c = CheckLib()
    vp = C.c_void_p
    c.L.hoh_entropy_bound.restype = C.c_size_t
    c.L.hoh_entropy_bound.argtypes = [C.c_size_t, C.c_size_t, C.c_uint32]
    c.L.hoh_encode_entropy.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_uint32, vp, C.c_size_t,
                                       C.POINTER(C.c_size_t)]
    r = np.random.default_rng(5)
    cases = []
    for rng in (256, 512):
        for lo in (0, 100, rng - K):
            cases.append((edge_stream(rng, lo, 4101, lo + rng)[0], rng))
        cases.append((r.integers(0, rng, 4101).astype(np.uint16), rng))
        cases.append((np.minimum(r.geometric(0.05, 4101) - 1, rng - 1).astype(np.uint16), rng))
        # an exact tie: two equal, separate peaks -> the lower one
        tie = np.repeat(np.array([10, 10 + 2 * K], np.uint16), 2048)
        cases.append((tie, rng))
    cases.append((np.zeros(100, np.uint16), 2))
    try:
        for sym, rng in cases:
            cap = c.L.hoh_entropy_bound(sym.size, rng, 15)
            out = np.empty(cap, np.uint8)
            n = C.c_size_t(0)
            rc = c.L.hoh_encode_entropy(c.h, sym.ctypes.data, sym.size, rng, 15, out.ctypes.data, cap, C.byref(n))
            assert rc == 0, rc
            assert out[:n.value].tobytes() == orc.encode_entropy(sym, rng, 15)
            st = c.streams(1)[0]
            assert st["fast"] == 1 and st["sizeonly"] == 0
            assert (int(st["wlo"]), int(st["whi"])) == window(orc, sym, rng), (rng, sym[:8])
    finally:
        c.close()


@pytest.fixture(scope="module")
def mixed():
    """768 x 512: 6 tiles, 18 plane chains in one wave; the tiles hold noise 0, 2, 4, 40, 4 and 40,
    with one flat block: lanes that always hit, sometimes miss and mostly miss share every lookup"""
    from hoh_ans.synth import synth_rgb
    img = synth_rgb(768, 512, seed=11, noise=4)
    for (tx, ty), nz in {(0, 0): 0, (1, 0): 2, (0, 1): 40, (2, 1): 40}.items():
        img[256 * ty:256 * ty + 256, 256 * tx:256 * tx + 256] = synth_rgb(256, 256, seed=20 + tx + 3 * ty, noise=nz)
    img[300:420, 300:480] = (17, 130, 250)
    return img


def test_mixed_lanes_one_wave(hoh, orc, ctxs, mixed):
    want = orc.choh(mixed)
    for name, ctx in ctxs.items():
        assert hoh.choh(mixed, ctx=ctx) == want, "CHAIN_TABLES %s" % name


def test_batch_equals_single(hoh, ctxs):
    import torch
    from hoh_ans.synth import synth_rgb
    W = H = 512
    imgs = [synth_rgb(W, H, seed=31 + i, noise=nz) for i, nz in enumerate((2, 8, 40))]
    single = [hoh.choh(im, ctx=ctxs["global"])[0] for im in imgs]
    rgb = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).cuda()
    stride = (hoh.lib().hoh_encode_bound(W, H) + 255) // 256 * 256
    for name, ctx in ctxs.items():
        out = torch.zeros(3 * stride, dtype=torch.uint8, device="cuda")
        st = torch.full((6,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        hoh.encode_images_async(rgb, 3, W, H, out, stride, st, ctx=ctx)
        torch.cuda.synchronize()
        s = st.cpu().numpy()
        for i in range(3):
            n = hoh.check_status(s[2 * i:2 * i + 2], "encode %d" % i)
            assert out[i * stride:i * stride + n].cpu().numpy().tobytes() == single[i], "CHAIN_TABLES %s, image %d" % (name, i)


def test_option_values(hoh):
    ctx = hoh.Context(0)
    try:
        for bad in (-1, 3):
            with pytest.raises(hoh.HohError):
                ctx.set_option(hoh.OPT_CHAIN_TABLES, bad)
    finally:
        ctx.close()
