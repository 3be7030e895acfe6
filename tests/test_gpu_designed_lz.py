"""GPU: the designed LZ tiles of tests/designed_lz.py at -s0..-s4 against the oracle, through the
posting lists (tiles of at most 65,536 positions: k_lzsort, k_lzvert, the four-segment k_lzscan)
and without them (300 x 260 and 256 x 300: k_lzcand, the serial walk); tests/test_designed_lz.py
pins what each tile holds and the oracle to the reference on these very tiles.

a. one tile per file (HOH_OPT_SMALL_IMAGES): header || the oracle's encode_tile, printed size;
b. four designs per tiled image against the oracle's choh; a batch against the single files;
c. the checking build's match list (pos, len, back) equals the oracle's streams, first difference
   reported -- a byte mismatch becomes a position, a length and a back;
d. its counters show that the path a design is for ran (k_lzscan's comment has the indices);
e. the other path on the same tile: forcing knobs, one child process each (knobs are read once);
f. the decoders read the same structures back (overlapping copies, b = 1 runs, vertical backs,
   the 65535 ceiling of decodable files).

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
for _p in (HERE, os.path.join(os.path.dirname(HERE), "hoh-ans_amd"), os.path.dirname(HERE)):   # the knob children import this module
    if _p not in sys.path:
        sys.path.insert(0, _p)

import designed_lz as D  # noqa: E402
from test_gpu_front_screen import TILE_DTYPE  # noqa: E402
from test_small_format import header  # noqa: E402

KEYS = sorted(D.designs())
IDS = ["%s-%s" % k for k in KEYS]
OPT_SMALL_IMAGES = 4
# counters of the checking build (k_lzscan, k_search.hip)
C_MEASURES, C_POSTING, C_RING, C_IMAGE, C_VERTICAL, C_STITCH = 0, 1, 3, 4, 7, 13
TILED = {"256x256": (512, 512, ["sweep", "stitch", "runs", "rowperiod9"]),
         "300x260": (600, 520, ["sweep", "vertical", "runs", "gaps"])}


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
def want_file():
    """(key, speed) -> the file a design should have"""
    D.warm(D.oracle_tile, D.tile_jobs())

    def f(key, speed):
        t = D.designs()[key]
        return header(t.w, t.h) + D.oracle_tile(key, speed)
    return f


@pytest.fixture(scope="module")
def want_matches():
    """(key, speed) -> the oracle's match list"""
    D.warm(D.oracle_lz, D.lz_jobs())
    return lambda key, speed: D.oracle_matches(key, D.SPEED_DIST[speed])


def tiled_image(shape):
    W, H, names = TILED[shape]
    tw, th = W // 2, H // 2
    img = np.zeros((H, W, 3), np.uint8)
    for k, name in enumerate(names):
        t = D.designs()[(name, shape)]
        assert (t.w, t.h) == (tw, th)
        img[(k // 2) * th:(k // 2 + 1) * th, (k % 2) * tw:(k % 2 + 1) * tw] = t.image()
    return img


def check_encode(c, torch, t, speed):
    """one tile through the checking build -> (file, [(pos, len, back & 0xffff)], counters)"""
    f = c.encode(torch.from_numpy(np.ascontiguousarray(t.image())).cuda().reshape(-1), t.w, t.h, speed, torch)
    nm = int(c.read(8, np.zeros(1, TILE_DTYPE))[0]["nmatch"])
    m = c.read(0, np.zeros(3 * max(nm, 1), np.uint32)).reshape(-1, 3)[:nm]
    dbg = c.read(5, np.zeros(64, np.uint32))
    return f, [(int(p), int(L), int(b) & 0xffff) for p, L, b in m], dbg[:16].tolist()


def first_difference(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return "match %d: got %s, want %s" % (i, a, b)
    if len(got) > len(want):
        return "%d matches, want %d; the first extra one: %s" % (len(got), len(want), got[len(want)])
    if len(got) < len(want):
        return "%d matches, want %d; the first missing one: %s" % (len(got), len(want), want[len(got)])
    return ""


# ---------------------------------------------------------------- a. one tile per file

@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_file_parity(hoh, sctx, want_file, key):
    t = D.designs()[key]
    for speed in D.speeds_of(t):
        want = want_file(key, speed)
        data, printed = hoh.choh(t.image(), ctx=sctx, speed=speed)
        assert printed == len(data) == len(want), speed
        assert data == want, speed


# ---------------------------------------------------------------- b. tiled and batched

@pytest.fixture(scope="module")
def want_tiled(orc):
    jobs = [(shape, speed) for shape in TILED for speed in (1, 2, 3, 4)]
    return dict(zip(jobs, D.warm(lambda shape, speed: orc.choh(tiled_image(shape), speed), jobs)))


@pytest.mark.parametrize("speed", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", sorted(TILED))
def test_tiled_parity(hoh, want_tiled, shape, speed):
    ref, ref_printed = want_tiled[(shape, speed)]
    data, printed = hoh.choh(tiled_image(shape), speed=speed)
    assert printed == ref_printed and len(data) == len(ref)
    assert data == ref


@pytest.mark.parametrize("speed", [1, 4])
def test_batch_equals_singles(hoh, sctx, want_file, speed):
    import torch
    keys = [k for k in KEYS if k[1] == "256x256"]
    n, W, H = len(keys), 256, 256
    rgb = torch.from_numpy(np.concatenate([D.designs()[k].image().reshape(-1) for k in keys])).cuda()
    stride = hoh.lib().hoh_encode_bound(W, H)
    out = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
    hoh.encode_images_async(rgb, n, W, H, out, stride, st, ctx=sctx, speed=speed)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    for i, k in enumerate(keys):
        want = want_file(k, speed)
        assert hoh.check_status(s[2 * i:2 * i + 2], "batch encode %s" % (k,)) == len(want), k
        assert out[i * stride:i * stride + len(want)].cpu().numpy().tobytes() == want, k


# ---------------------------------------------------------------- c, d. match lists and paths (checking build)

@pytest.fixture(scope="module")
def check():
    import torch  # noqa: F401
    from checklib import CheckLib
    c = CheckLib()
    c.set_option(OPT_SMALL_IMAGES, 1)
    yield c
    c.close()


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_match_lists_and_paths(check, want_file, want_matches, key):
    import torch
    t = D.designs()[key]
    name, posting = key[0], t.n <= 65536
    for speed in D.speeds_of(t):
        f, got, dbg = check_encode(check, torch, t, speed)
        want = want_matches(key, speed)
        assert got == want, (speed, first_difference(got, want))
        assert f == want_file(key, speed), speed
        if speed == 0:
            continue                                              # k_lz: the counters are k_lzscan's
        print(key, speed, "measures %d posting %d ring %d image %d vertical %d stitch %d" % tuple(
            dbg[i] for i in (C_MEASURES, C_POSTING, C_RING, C_IMAGE, C_VERTICAL, C_STITCH)))
        if name == "sweep":
            assert dbg[C_RING] > 0 and dbg[C_IMAGE] > 0, (speed, dbg)
        if name == "vertical":
            assert dbg[C_VERTICAL] > 0, (speed, dbg)
        if name == "stitch":
            assert dbg[C_STITCH] > 0, (speed, dbg)
        if name.startswith("rowperiod"):
            assert dbg[C_POSTING] > dbg[C_MEASURES], (speed, dbg)
        if not posting:
            assert dbg[C_POSTING] == 0, (speed, dbg)


# ---------------------------------------------------------------- e. the other path on the same tile

_KNOB_CHILD = r"""
import hashlib, json, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import designed_lz as D
import test_gpu_designed_lz as S
from checklib import CheckLib
c = CheckLib()
c.set_option(S.OPT_SMALL_IMAGES, 1)
res = {}
for key, t in sorted(D.designs().items()):
    for speed in D.speeds_of(t):
        if speed:
            f, m, dbg = S.check_encode(c, torch, t, speed)
            res["%s %s %d" % (key[0], key[1], speed)] = {"sha": hashlib.sha256(f).hexdigest(), "m": m, "dbg": dbg}
c.close()
print("RESULT " + json.dumps(res))
"""

KNOBS = {"no-posting": {"HOH_LZ_POSTING": "0"}, "one-segment": {"HOH_LZS_SEG": "1"},
         "rings-2048-1024": {"HOH_LZS_RING_MAX": "2048", "HOH_LZS_RING_HI": "1024"},
         "sort-512": {"HOH_LZSORT_HALF_SPEED": "1"}, "sort-1024": {"HOH_LZSORT_HALF_SPEED": "5"}}


def test_both_paths_under_knobs(want_file, want_matches):
    """every forcing knob in a process of its own, side by side: the same files and match lists"""
    procs = {k: subprocess.Popen([sys.executable, "-c", _KNOB_CHILD, HERE], env=dict(os.environ, HOH_QUIET="1", **env),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k, env in KNOBS.items()}
    outs = {k: p.communicate(timeout=100) + (p.returncode,) for k, p in procs.items()}
    for k, (so, se, rc) in outs.items():
        assert rc == 0, (k, se[-3000:])
        res = json.loads([ln for ln in so.splitlines() if ln.startswith("RESULT ")][-1][7:])
        assert len(res) == sum(1 for _, sp in D.tile_jobs() if sp)
        for key, t in sorted(D.designs().items()):
            for speed in D.speeds_of(t):
                if not speed:
                    continue
                r = res["%s %s %d" % (key[0], key[1], speed)]
                got, want = [tuple(m) for m in r["m"]], want_matches(key, speed)
                assert got == want, (k, key, speed, first_difference(got, want))
                assert r["sha"] == hashlib.sha256(want_file(key, speed)).hexdigest(), (k, key, speed)
                if k == "no-posting":
                    assert r["dbg"][C_POSTING] == 0, (k, key, speed)
                if k == "one-segment":
                    assert r["dbg"][C_STITCH] == 0, (k, key, speed)


# ---------------------------------------------------------------- f. the decoders on the same structures

@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_decodable_round_trip(hoh, dctx, key):
    t = D.designs()[key]
    for speed in (0, 1, 4):
        if speed in D.speeds_of(t):
            data, printed = hoh.choh(t.image(), ctx=dctx, speed=speed)
            assert printed == len(data), speed
            assert np.array_equal(hoh.dhoh(data, ctx=dctx), t.image()), speed


def test_plain_s0_round_trip(hoh, sctx, want_file):
    for key in KEYS:
        t = D.designs()[key]
        if 0 in D.speeds_of(t):                                   # the palette tiles carry no palette (Q15)
            assert np.array_equal(hoh.dhoh(want_file(key, 0), ctx=sctx), t.image()), key
