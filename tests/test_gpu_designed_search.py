"""GPU: the designed planes and images of tests/designed_search.py (tests/test_designed_search.py pins
what each one reaches) through the -s1..-s4 predictor search and prob_bits ladder, against the
oracle's report of the same decisions.

a. whole files: plain, OPT_SMALL_IMAGES (the one tile of an untiled image) and OPT_DECODABLE; the
   decodable files are parsed (tests/decodable_ref.py): every layer's predictor map is the report's,
   its prob_bits the decodable ladder's choice on the report's sizes, and they decode to the image;
b. the checking build's search scratch (hoh_debug_read 9): per searched plane the entropy tables
   and every mask cost of every cell and pass equal the report's float64 bit for bit
   (k_search.hip's own claim: the reference's sums in the reference's order), and the predictor
   map k_search's last pass wrote (hoh_debug_read 10, 11) is the report's;
c. the ladder's StreamInfo records: kept trials have the report's sizes, pruned ones lie strictly
   above the winner and their lower bound holds, the final stream is the report's; and unpruned
   (HOH_LADDER_PRUNE=0, a child process: knobs are read once) all eight sizes, the word bounds,
   the same files;
d. the plane-level entry points on every plane: launch_search_plane (k_search_costs, k_search_pick:
   another walk and another pick loop).  That path's ladder is a loop on the host
   (hoh_plane_s.cpp); k_prune_s and k_choose_s run for images only, so c. asserts per image which
   ladder outcome its designed plane reaches.

Every oracle answer is computed once per module, several at a time."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "hoh-ans_amd"), os.path.dirname(HERE)):   # the child imports this module
    if _p not in sys.path:
        sys.path.insert(0, _p)

import decodable_ref as dr  # noqa: E402
import designed_search as D  # noqa: E402
from checklib import KS_FIN, KS_MED, KS_VAR, SM_EMPTY, SPT_S, VAR_PB  # noqa: E402

OPT_SMALL_IMAGES = 4
IMAGES = list(D.IMAGE_NAMES)
PLANES = sorted(D.planes())


@pytest.fixture(scope="module")
def hoh():
    import torch  # noqa: F401  (before the first context: torch brings its own HIP runtime)
    import hoh_ans
    return hoh_ans


@pytest.fixture(scope="module")
def sctx(hoh):
    c = hoh.Context(0)
    c.set_option(hoh.OPT_SMALL_IMAGES, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dctx(hoh):
    c = hoh.Context(0)
    c.set_option(hoh.OPT_SMALL_IMAGES, 1)
    c.set_option(hoh.OPT_DECODABLE, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def check():
    import torch  # noqa: F401
    from checklib import CheckLib
    c = CheckLib()
    c.set_option(OPT_SMALL_IMAGES, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want_file():
    D.warm(D.image_file, [(n, sp) for n in IMAGES for sp in D.SPEEDS])
    return D.image_file


@pytest.fixture(scope="module")
def want_report():
    D.warm(D.tile_report, D.report_jobs())
    return D.tile_report


@pytest.fixture(scope="module")
def plane_report():
    D.warm(D.report, [(n, sp) for n in PLANES for sp in D.SPEEDS])
    return D.report


def untiled(name):
    return len(D.tiles_of(D.images()[name])) == 1


# ---------------------------------------------------------------- a. whole files

@pytest.mark.parametrize("name", IMAGES)
def test_files(hoh, orc, sctx, want_file, name):
    img = D.images()[name]
    for sp in D.SPEEDS:
        want = want_file(name, sp)
        if isinstance(want, orc.OracleError):
            assert want.code == -4, want
            for ctx in (None, sctx):
                with pytest.raises(hoh.HohError) as g:
                    hoh.choh(img, ctx=ctx, speed=sp)
                assert g.value.code == 5
            continue
        plain, printed, whole = want
        data, gp = hoh.choh(img, speed=sp)
        assert gp == printed and data == plain, sp
        if untiled(name):
            data, gp = hoh.choh(img, ctx=sctx, speed=sp)
            assert gp == len(data) == len(whole), sp
            assert data == whole, sp


@pytest.mark.parametrize("name", IMAGES)
def test_decodable_files(hoh, dctx, want_report, name):
    """the decodable file's layers carry the report's maps and the decodable ladder's choice"""
    img = D.images()[name]
    H, W, _ = img.shape
    for sp in D.SPEEDS:
        data, printed = hoh.choh(img, ctx=dctx, speed=sp)
        assert printed == len(data), sp
        assert np.array_equal(hoh.dhoh(data, ctx=dctx), img), sp
        tiles = dr.tiles_of(data)[2] if not untiled(name) else [(0, 0, W, H, len(D.header(W, H)), len(data))]
        for k, (x0, y0, w, h, s, e) in enumerate(tiles):
            if data[s + 2] not in (128, 2):
                assert name == "palette256"                       # the indexed mode: not parsed here
                continue
            t = dr.parse_tile(data, s, e, w, h)
            planes = [0, 1, 2] if t["mode"] == 128 else [0, 4, 5]
            for L, p in zip(t["layers"], planes):
                r = want_report(name, k, p, sp)
                assert (L["xt"], L["yt"]) == (r["xt"], r["yt"])
                got = [L["masks"][i] for i in L["pidx"]]
                assert got == [D.MASKS[i] for i in r["pidx"][-1]], (sp, k, p)
                pb = D.decodable_choice(r)
                assert len(L["stream"]) == r["size"][pb], (sp, k, p, pb, L["pb"])
                assert L["pb"] in (None, pb), (sp, k, p)           # None: a stored stream


def _batch(hoh, ctx, names, W, H, speed):
    import torch
    n = len(names)
    rgb = torch.from_numpy(np.concatenate([D.images()[k].reshape(-1) for k in names])).cuda()
    stride = hoh.lib().hoh_encode_bound(W, H)
    out = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
    hoh.encode_images_async(rgb, n, W, H, out, stride, st, ctx=ctx, speed=speed)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    return [(hoh.check_status(s[2 * i:2 * i + 2], "batch encode %s" % k),
             out[i * stride:(i + 1) * stride].cpu().numpy()) for i, k in enumerate(names)]


@pytest.mark.parametrize("speed", [2, 3])
def test_batched(hoh, sctx, want_file, speed):
    """the 256 x 256 designs in one batched call, the 511 x 511 one (twice) in another"""
    names = [n for n in IMAGES if D.images()[n].shape[:2] == (256, 256) and n != "palette256"]
    assert len(names) >= 6
    for (n, buf), name in zip(_batch(hoh, sctx, names, 256, 256, speed), names):
        want = want_file(name, speed)[2]
        assert n == len(want) and buf[:n].tobytes() == want, name
    want = want_file("lad_up511", speed)[2]
    for n, buf in _batch(hoh, sctx, ["lad_up511", "lad_up511"], 511, 511, speed):
        assert n == len(want) and buf[:n].tobytes() == want


# ---------------------------------------------------------------- b, c. the checking build

def _encode_check(c, torch, name, sp):
    img = D.images()[name]
    H, W, _ = img.shape
    return c.encode(torch.from_numpy(np.ascontiguousarray(img)).cuda().reshape(-1), W, H, sp, torch)


@pytest.mark.parametrize("name", IMAGES)
def test_search_scratch_bit_exact(check, want_file, want_report, name):
    import torch
    nt = len(D.tiles_of(D.images()[name]))
    for sp in D.SPEEDS:
        want = want_file(name, sp)
        f = _encode_check(check, torch, name, sp)
        assert f == want[2], sp
        npass = 2 if sp > 2 else 1
        ent, cost = check.search_scratch(nt, npass)
        pinfo, maps = check.search_maps(nt)
        for k in range(nt):
            for p in D.searched_planes(name, k, sp):
                r = want_report(name, k, p, sp)
                T, npred = r["ncell"], r["npred"]
                assert r["npass"] == npass and npred == D.NPRED[sp]
                for ps in range(npass):
                    # after pass 0 of -s3 / -s4 the table is already the refined one (pass 1's); the
                    # kernel writes the plane's 2^depth entries, the rest of the slot is whatever
                    # the buffer held before
                    rng = 512 if p in (1, 2) else 256
                    assert np.array_equal(ent[ps, k, p, :rng], r["ent"][-1 if npass == 2 else 0][:rng]), (sp, k, p, ps)
                    got, ref = cost[ps, k, p, :T, :npred], r["cost"][ps][:, :npred]
                    bad = np.argwhere(got != ref)
                    assert not bad.size, "-s%d tile %d plane %d pass %d: %d costs differ, first (cell, mask) %s: %r != %r" % (
                        sp, k, p, ps, len(bad), bad[0].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
                # the map k_search's pick loop chose in its last pass, as the kernel wrote it (pass 0's
                # map at -s3 / -s4 lives in LDS only: the refined table above is counted under it)
                assert (int(pinfo[k, p]["xt"]), int(pinfo[k, p]["yt"])) == (r["xt"], r["yt"]), (sp, k, p)
                assert np.array_equal(maps[k, p, :T], r["pidx"][-1]), (sp, k, p)


def ladder_check(st, r, where, unpruned=False):
    """st: the SPT_S StreamInfo records of one tile; r: the report of plane p = where[-1]"""
    p = where[-1]
    v = st[KS_VAR + p * 8:KS_VAR + p * 8 + 8]
    med, fin = st[KS_MED + p], st[KS_FIN + p]
    assert int(med["size"]) == r["med_size"], where
    assert [int(x) for x in v["pb"]] == list(VAR_PB), where
    taken = {16, 15} | ({17, 18, 19} if r["branch"] > 0 else {14, 13, 12})
    assert (r["size"][16] < r["size"][15]) == (r["branch"] > 0)
    for k in range(8):
        pb, so = VAR_PB[k], int(v[k]["sizeonly"])
        assert int(v[k]["err"]) == 0 and so in ((1, 3) if unpruned else (1, 2, 3)), (where, pb, so)
        if so == 2:
            # pruned: its lower bound holds, and among the trials the ladder compares (the 16/15 pair
            # and the three of the branch it takes) it lies strictly above the winner.  The three of
            # the other branch are never compared (k_choose_s), so they may be pruned below it -- wrap8
            # at -s2: 16 < 15, 21,687 bytes kept, prob_bits 14 at 21,570 not encoded -- once the
            # pair's order is certain: the pair's sizes below (exact, or a bound on the certain side)
            assert int(v[k]["size"]) <= r["size"][pb], (where, pb)
            # (prob_bits 16 itself is only ever compared with 15: pruned, it is at least 15's size, so at
            # least the winner's -- lad_equal: every size is the stored 4,105 and 16 is not encoded)
            if pb == 16 and r["branch"] < 0:
                assert r["size"][16] >= r["size"][15] >= r["possible"], (where, r["size"], r["possible"])
            elif pb in taken:
                assert r["size"][pb] > r["possible"], (where, pb, r["size"][pb], r["possible"])
            else:
                assert (int(v[0]["size"]) < int(v[1]["size"])) == (r["branch"] > 0), where
        else:
            assert int(v[k]["size"]) == r["size"][pb], (where, pb, int(v[k]["size"]), r["size"][pb])
            if int(v[k]["whi"]) >= int(v[k]["wlo"]) >= 2 and int(v[k]["words"]) > 0:
                assert int(v[k]["wlo"]) <= int(v[k]["words"]) <= int(v[k]["whi"]), (where, pb)
    if r["winner"] > 0:                                         # a trial won: the final stream is its
        assert int(fin["pb"]) == r["winner"] and int(fin["size"]) == r["possible"], where
        assert r["valid"] and not r["stale"]
    else:                                                       # the MED stream, whole or cut (Q14)
        assert int(fin["mode"]) == SM_EMPTY and int(fin["n"]) == 0, where
        assert r["valid"] and r["possible"] <= r["med_size"] and r["stale"] == (r["possible"] < r["med_size"]), where
        if p == 0 and not int(med["drop"]):
            assert int(med["clip"]) == r["possible"], where


@pytest.mark.parametrize("name", IMAGES)
def test_ladder_records(check, want_file, want_report, name):
    import torch
    nt = len(D.tiles_of(D.images()[name]))
    pruned = 0
    for sp in D.SPEEDS:
        f = _encode_check(check, torch, name, sp)
        assert f == want_file(name, sp)[2], sp
        st = check.streams(nt * SPT_S).reshape(nt, SPT_S)
        for k in range(nt):
            for p in D.searched_planes(name, k, sp):
                ladder_check(st[k], want_report(name, k, p, sp), (name, sp, k, p))
                pruned += int((st[k][KS_VAR + p * 8:KS_VAR + p * 8 + 8]["sizeonly"] == 2).sum())
    print(name, "pruned trials over -s1..-s4: %d" % pruned)
    # what k_prune_s / k_choose_s were shown: the designed plane's outcome in this image is the
    # plane's own (tests/test_designed_search.py), and over the images every required one occurs
    P = D.planes()
    if name in P and P[name].want:
        k = 0 if P[name].depth == 8 else 1
        for sp in D.SPEEDS:
            want = P[name].want.get(sp) if isinstance(P[name].want, dict) else P[name].want
            if want:
                assert D.outcome(want_report(name, 0, k, sp)) == want, (name, sp)


def test_ladder_outcomes_reached_by_images(want_report):
    seen = {}
    for j in D.report_jobs():
        seen.setdefault(D.outcome(want_report(*j)), []).append(j)
    print({o: len(v) for o, v in seen.items()})
    for o in (("med",), ("win", 12), ("win", 13), ("win", 14), ("stale",), ("equal",), ("up", 17), ("up-stale",)):
        assert o in seen, o
    r = want_report("lad_onebyte", 0, 0, 1)                   # and the one-byte win among them
    assert r["possible"] == r["size"][13] == r["med_size"] - 1


_UNPRUNED_CHILD = r"""
import hashlib, json, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import designed_search as D
import test_gpu_designed_search as S
from checklib import CheckLib, SPT_S
c = CheckLib()
c.set_option(S.OPT_SMALL_IMAGES, 1)
res = {}
for name in S.IMAGES:
    nt = len(D.tiles_of(D.images()[name]))
    for sp in D.SPEEDS:
        f = S._encode_check(c, torch, name, sp)
        st = c.streams(nt * SPT_S)
        res["%s %d" % (name, sp)] = {"sha": hashlib.sha256(f).hexdigest(),
                                     "st": {k: st[k].astype(np.int64).tolist() for k in
                                            ("size", "pb", "sizeonly", "err", "wlo", "whi", "words", "mode", "n", "drop", "clip")}}
c.close()
print("RESULT " + json.dumps(res))
"""


def test_ladder_unpruned(want_file, want_report):
    """HOH_LADDER_PRUNE=0 in a fresh process: no trial is pruned, all eight sizes are the report's,
    wlo <= words <= whi for every bounded trial of every design, the files are unchanged"""
    env = dict(os.environ, HOH_LADDER_PRUNE="0", HOH_QUIET="1")
    p = subprocess.run([sys.executable, "-c", _UNPRUNED_CHILD, HERE], env=env, capture_output=True, text=True,
                       timeout=100)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    from checklib import STREAM_DTYPE
    bounded = 0
    for name in IMAGES:
        nt = len(D.tiles_of(D.images()[name]))
        for sp in D.SPEEDS:
            r = res["%s %d" % (name, sp)]
            assert r["sha"] == hashlib.sha256(want_file(name, sp)[2]).hexdigest(), (name, sp)
            st = np.zeros(nt * SPT_S, STREAM_DTYPE)
            for key, val in r["st"].items():
                st[key] = val
            st = st.reshape(nt, SPT_S)
            assert not (st["sizeonly"] == 2).any(), (name, sp)
            for k in range(nt):
                for pl in D.searched_planes(name, k, sp):
                    ladder_check(st[k], want_report(name, k, pl, sp), (name, sp, k, pl), unpruned=True)
                    v = st[k][KS_VAR + pl * 8:KS_VAR + pl * 8 + 8]
                    bounded += int(((v["whi"] >= v["wlo"]) & (v["wlo"] >= 2) & (v["words"] > 0)).sum())
    print("bounded trials checked: %d" % bounded)
    assert bounded > 500


# ---------------------------------------------------------------- d. the plane-level path

@pytest.mark.parametrize("name", PLANES)
def test_plane_level(hoh, orc, plane_report, name):
    p = D.planes()[name]
    for sp in D.SPEEDS:
        r = plane_report(name, sp)
        if r["error"]:
            with pytest.raises(hoh.HohError) as g:
                hoh.layer_encode(p.d, p.depth, p.nuke, speed=sp)
            assert g.value.code == 5 and r["error"] == -4
            continue
        got = hoh.layer_encode(p.d, p.depth, p.nuke, speed=sp)
        assert len(got) == len(r["layer"]) and got == r["layer"], sp
        for ps in range(r["npass"] if sp < 4 else 0):            # the oracle's maps of both passes (-s4's are -s3's)
            tm = np.array([D.MASKS[i] for i in r["pidx"][ps]], np.uint16)
            res = orc.predict_all(p.d, p.depth, r["xt"], r["yt"], tm)
            assert np.array_equal(hoh.predict_all(p.d, p.depth, r["xt"], r["yt"], tm), res), (sp, ps)
            assert np.array_equal(hoh.unpredict_all(res, p.w, p.h, p.depth, r["xt"], r["yt"], tm), p.d), (sp, ps)
        if sp == 4:
            assert all(np.array_equal(a, b) for a, b in zip(r["pidx"], plane_report(name, 3)["pidx"]))
