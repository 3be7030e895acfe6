"""CPU: the oracle's report (oracle.layer_report) against the reference, and every claim of
tests/designed_search.py against the report -- before tests/test_gpu_designed_search.py uses the
planes.  Run with -s to see the measured counts."""
import math

import numpy as np
import pytest

import oracle as O

import designed_lz as DL
import designed_search as D

pytestmark = pytest.mark.skipif(O.ref() is None, reason="oracle/_ref not built (no /root/reference)")
JOBS = [(n, sp) for n in D.planes() for sp in D.SPEEDS]


@pytest.fixture(scope="module")
def reports():
    D.warm(D.report, JOBS)
    return D.report


def union_masks(reports, names, speed):
    u = set()
    for n in names:
        u |= set(reports(n, speed)["pidx"].reshape(-1).tolist())
    return u


# ------------------------------------------------------------------ 1. the report is the reference's

def test_report_layer_is_the_references(reports):
    """or_layer_report's bytes are or_layer_encode's (one code) and the reference's layer_encode's"""
    R = O.ref()
    for name, sp in JOBS:
        p, r = D.planes()[name], reports(name, sp)
        assert r["error"] == 0, (name, sp, r["error"])
        assert r["layer"] == O.layer_encode(p.d, p.depth, sp, p.nuke), (name, sp)
        nuke = np.zeros((p.h, p.w), np.uint8) if p.nuke is None else p.nuke
        out = np.empty(len(r["layer"]) + (1 << 20), np.uint8)
        n = R.ref_layer_encode(p.d.ctypes.data_as(O.u16p), p.w * p.h, p.w, p.h, p.depth, sp,
                               nuke.ctypes.data_as(O.u8p), out.ctypes.data_as(O.u8p))
        assert out[:n].tobytes() == r["layer"], (name, sp)


@pytest.mark.parametrize("name,sp", [("planted256", 1), ("planted256", 2), ("planted256", 3), ("planted300", 4),
                                     ("planted100", 2), ("colconst", 3), ("wrap9", 3), ("lad_stale15", 3)])
def test_report_costs_from_the_references_residuals(reports, name, sp):
    """entropy tables from the definition (layer_encode.hpp:133-147), and every mask cost recomputed
    from ref_channelpredict_section's residuals by a sequential float loop (numpy.sum is pairwise):
    equal bit for bit.  The chosen index is the first of least cost; pass 1's table comes from
    channelpredict_all under pass 0's map."""
    R = O.ref()
    p, r = D.planes()[name], reports(name, sp)
    n, T, npred = p.w * p.h, r["ncell"], r["npred"]
    assert (T, npred, r["npass"]) == (p.cells, D.NPRED[sp], 2 if sp > 2 else 1)
    res = O.predict_fastpath(p.d, p.depth).reshape(-1)
    buf = np.empty(n, np.uint16)
    for ps in range(r["npass"]):
        fr = 1 + np.bincount(res, minlength=1 << p.depth)
        table = np.zeros(512)
        table[:1 << p.depth] = [-math.log2(float(f) / float(n)) for f in fr.tolist()]   # the C library's log2
        assert np.array_equal(table, r["ent"][ps]), (name, sp, ps)
        for cell in range(T):
            best, bi = 99999999999.0, 0
            for m in range(npred):
                k = R.ref_channelpredict_section(p.d.ctypes.data_as(O.u16p), p.w, p.h, p.depth, r["xt"], r["yt"],
                                                 cell % r["xt"], cell // r["xt"], D.MASKS[m], buf.ctypes.data_as(O.u16p))
                s = 0.0
                for v in table[buf[:k]].tolist():
                    s += v
                assert s == r["cost"][ps][cell][m], (name, sp, ps, cell, m, s, r["cost"][ps][cell][m])
                if s < best:
                    best, bi = s, m
            assert bi == r["pidx"][ps][cell], (name, sp, ps, cell)
        tm = np.array([D.MASKS[i] for i in r["pidx"][ps]], np.uint16)
        res = np.empty(n, np.uint16)
        R.ref_channelpredict_all(p.d.ctypes.data_as(O.u16p), p.w, p.h, p.depth, r["xt"], r["yt"],
                                 tm.ctypes.data_as(O.u16p), res.ctypes.data_as(O.u16p))


def test_report_sizes_are_stream_sizes(reports):
    """the ladder sizes are the streams' of the final residuals (the plane's own nuke mask applied)"""
    for name in ("planted100", "lad_13", "lad_nuke90", "lad_nukeall", "wrap9"):
        p = D.planes()[name]
        for sp in (1, 3):
            r = reports(name, sp)
            tm = np.array([D.MASKS[i] for i in r["pidx"][-1]], np.uint16)
            res = O.predict_all(p.d, p.depth, r["xt"], r["yt"], tm)
            med = O.predict_fastpath(p.d, p.depth).reshape(-1)
            if p.nuke is not None:
                keep = p.nuke.reshape(-1) == 0
                res, med = res[keep], med[keep]
            assert r["med_size"] == len(O.encode_entropy(med, 1 << p.depth, 15))
            for pb in range(12, 20):
                assert r["size"][pb] == len(O.encode_entropy(res, 1 << p.depth, pb)), (name, sp, pb)


# ------------------------------------------------------------------ 2. the designs' claims

def test_planted_pixels():
    first, tie = D.pixels("planted256")
    cnt = np.bincount(first.reshape(-1), minlength=16)
    print("planted256: first-least counts %s, equal two smallest errors %.1f%%" % (cnt.tolist(), 100 * tie.mean()))
    assert all(cnt[e] >= 1000 for e in range(1, 9)), cnt.tolist()
    assert tie.mean() >= 0.25
    for name, p in D.planes().items():                        # Paeth equals L, T or TL, which come first
        assert np.bincount(D.pixels(name)[0].reshape(-1), minlength=16)[9] == 0, name


def test_pixel_report_is_the_references_walk():
    """the first-least predictor of the report is the best predictor channelpredict_all keeps under
    the all-sixteen mask: the reference's residuals follow from it (inner pixels: both neighbours'
    best predictors come from the walk itself; the last row keeps 0 instead)"""
    R = O.ref()
    for name in ("planted256", "planted300", "wrap8"):
        p = D.planes()[name]
        first, _ = D.pixels(name)
        tm = np.array([0xffff], np.uint16)
        res = np.empty(p.w * p.h, np.uint16)
        R.ref_channelpredict_all(p.d.ctypes.data_as(O.u16p), p.w, p.h, p.depth, 1, 1, tm.ctypes.data_as(O.u16p),
                                 res.ctypes.data_as(O.u16p))
        res = res.reshape(p.h, p.w).astype(np.int64)
        d, c = p.d.astype(np.int64), 1 << p.depth
        y, x = [a.reshape(-1) for a in np.mgrid[1:p.h - 1, 1:p.w - 1]]
        pr = D.preds(d[y, x - 1], d[y - 1, x], d[y - 1, x - 1], d[y - 1, x + 1])
        k = np.arange(y.size)
        want = (d[y, x] - D._midp(pr[first[y - 1, x], k], pr[first[y, x - 1], k]) + c // 2 + c) % c
        assert np.array_equal(res[y, x], want), name


def test_planted_masks(reports):
    names = [n for n, p in D.planes().items() if p.group == "planted"]
    got = {sp: union_masks(reports, names, sp) for sp in D.SPEEDS}
    for sp in D.SPEEDS:
        print("planted planes, -s%d: %d masks chosen %s" % (sp, len(got[sp]), sorted(got[sp])))
        for n in names:
            print("    %s: %s" % (n, sorted(set(reports(n, sp)["pidx"].reshape(-1).tolist()))))
    assert len(got[1]) == 5
    assert len(got[2]) >= 8
    assert len(got[3]) >= 11 and len(got[4]) >= 11
    every = set()
    for sp in D.SPEEDS:
        every |= union_masks(reports, list(D.planes()), sp)
    print("all planes: masks chosen %s" % sorted(every))
    assert every == set(range(13))                            # 13 (all sixteen) ties with 12 and comes second
    for name, sp in JOBS:                                     # ... on every cell of every plane
        c = reports(name, sp)["cost"]
        if c.shape[1] and sp > 2:
            assert np.array_equal(c[:, :, 12], c[:, :, 13]), (name, sp)


def test_exact_ties(reports):
    for name in ("flat", "rowconst", "colconst"):
        for sp in D.SPEEDS:
            r = reports(name, sp)
            tied = [D.tied_cells(r, k) for k in range(r["npass"])]
            print("%s -s%d: %s of %d cells tie at the minimum, chosen %s" % (
                name, sp, tied, r["ncell"], sorted(set(r["pidx"].reshape(-1).tolist()))))
            assert r["ncell"] == 49 and min(tied) >= 40, (name, sp, tied)
            for k in range(r["npass"]):                       # the first of the tied masks is the one chosen
                c = r["cost"][k][:, :r["npred"]]
                assert np.array_equal(np.argmin(c, axis=1), r["pidx"][k]), (name, sp, k)
    for sp in D.SPEEDS:                                       # a later index than 0 wins a tie
        r = reports("colconst", sp)
        c = r["cost"][-1][:, :r["npred"]]
        tiedc = (c == c.min(axis=1, keepdims=True)).sum(axis=1) > 1
        assert (r["pidx"][-1][tiedc] > 0).sum() >= 40, sp


def test_near_ties(reports):
    found = {(n, sp): D.near_ties(reports(n, sp)) for n, sp in JOBS}
    found = {k: v for k, v in found.items() if v}
    print("cells whose two best costs differ by less than 1e-9 relative: %s" % found)
    assert ("lad_stale15", 3) in found and len(found[("lad_stale15", 3)]) >= 4


def test_wrap_planes():
    for name in ("wrap8", "wrap9"):
        p = D.planes()[name]
        c, d = 1 << p.depth, p.d.astype(np.int64)
        g = d[:-1, 1:] + d[1:, :-1] - d[:-1, :-1]              # T + L - TL
        res = O.predict_fastpath(p.d, p.depth).astype(np.int64) - c // 2
        print("%s: values %d..%d, T + L - TL below 0 at %d pixels, past the range at %d; |MED residual| > %d at %d" % (
            name, d.min(), d.max(), (g < 0).sum(), (g >= c).sum(), c // 4, (np.abs(res) > c // 4).sum()))
        assert d.min() <= 1 and d.max() == c - 1
        assert (g < 0).sum() >= 500 and (g >= c).sum() >= 500


def test_refine_changes_the_map(reports):
    for name in ("smooth256", "wrap8", "wrap9"):
        r = reports(name, 3)
        diff = int((r["pidx"][0] != r["pidx"][1]).sum())
        print("%s -s3: pass 1 differs from pass 0 in %d of %d cells" % (name, diff, r["ncell"]))
        assert diff >= 3


def test_ladder_outcomes(reports):
    seen = set()
    for name, p in D.planes().items():
        for sp in D.SPEEDS:
            r = reports(name, sp)
            o = D.outcome(r)
            seen.add(o)
            want = p.want.get(sp) if isinstance(p.want, dict) else p.want
            if want:
                print("%s -s%d: %s, MED %d, sizes %s, %d bytes kept" % (name, sp, o, r["med_size"],
                                                                        [r["size"][k] for k in range(12, 20)], r["possible"]))
                assert o == want, (name, sp, o, want)
    print("ladder outcomes over all planes: %s" % sorted(seen))
    for sp in D.SPEEDS:
        r = reports("lad_onebyte", sp)                        # the winner beats the next size by one byte
        others = [r["med_size"]] + [r["size"][k] for k in (15, 14, 12)]
        assert r["possible"] == r["size"][13] == min(others) - 1, (sp, r["size"], r["med_size"])
        r = reports("lad_stale15", sp)                        # 15's size cuts the (valid) MED stream
        assert r["valid"] and r["winner"] == 0 and r["possible"] == r["size"][15] < r["med_size"], sp
        r = reports("lad_equal", sp)
        assert set(r["size"].values()) == {r["med_size"]} and r["med_size"] == 2 + 2 + 1 + 4100   # stored
        r = reports("lad_up511", sp)
        assert r["branch"] == 1 and r["size"][16] < r["size"][15]
    r = reports("lad_14tie12", 1)                             # an exact tie: 14 is tried first and stays
    assert r["size"][14] == r["size"][12] == r["possible"]
    r = reports("wrap8", 2)                                   # the upward branch's own stale prefix
    assert D.outcome(r) == ("up-stale",) and r["possible"] == r["size"][16] < min(r["med_size"], r["size"][15])
    p = D.planes()["lad_nuke90"]
    assert p.nuke.mean() > 0.9
    assert D.planes()["lad_nukeall"].nuke.all() and reports("lad_nukeall", 4)["error"] == 0


# ------------------------------------------------------------------ 3. the images

def test_images(reports):
    imgs = D.images()
    tiles = [(n, k, t) for n, im in imgs.items() for k, t in enumerate(D.tiles_of(im))]

    for n, k, (x0, y0, w, h) in tiles:
        px = np.ascontiguousarray(imgs[n][y0:y0 + h, x0:x0 + w])
        cc = O.lib().or_count_colours(px.ctypes.data_as(O.u8p), px.size)
        assert not (np.array_equal(px[:, :, 0], px[:, :, 1]) and np.array_equal(px[:, :, 0], px[:, :, 2])), n
        if n == "palette256":
            assert 32 < cc <= 256, cc                          # a palette candidate, no LZ bonus
        else:
            assert cc == -1, (n, k, cc)
            assert D.windows_distinct(px), (n, k)              # no LZ match takes a design pixel away
    px = imgs["planted256"]                                    # ... which is what the oracle's search finds
    assert not DL.find_lz(O.lib().or_find_lz_rgb, px, 256, 256, 14, 0)[1].any()
    P = D.planes()
    for n, im in imgs.items():                                 # the designs sit in the planes the encoder searches
        pl = D.image_planes(im)
        if n in P and P[n].depth == 8:
            assert np.array_equal(pl[0][0], P[n].d), n
        elif n in P:
            assert np.array_equal(pl[1][0], P[n].d), n
    big = imgs["planted770"]
    tl = D.tiles_of(big)
    assert len(tl) == 6 and sorted({w * h for _, _, w, h in tl}) == sorted({257 * 258, 256 * 258, 257 * 257, 256 * 257})
    for sp in (1, 3):                                          # what the oracle reports for the image's own planes
        u = set()
        for k, (x0, y0, w, h) in enumerate(tl):
            d, depth = D.image_planes(big[y0:y0 + h, x0:x0 + w])[0 if k % 2 == 0 else 1]
            u |= set(O.layer_report(d, depth, sp)["pidx"].reshape(-1).tolist())
        print("planted770 -s%d: masks chosen in the six designed planes %s" % (sp, sorted(u)))
        assert len(u) >= (5 if sp == 1 else 9)
    both = D.image_planes(imgs["planted_both"])
    for pi in (0, 1):
        u = set(O.layer_report(both[pi][0], both[pi][1], 3)["pidx"].reshape(-1).tolist())
        print("planted_both plane %d -s3: masks %s" % (pi, sorted(u)))
        assert len(u) >= 6
    idx = D.palette_plane(imgs["palette256"])
    assert int(idx.max()) < 256
    print("palette256: %d colours, masks of the indexed plane at -s3 %s" % (
        int(idx.max()) + 1, sorted(set(O.layer_report(idx, 8, 3)["pidx"].reshape(-1).tolist()))))
