"""CPU: the designed LZ tiles (tests/designed_lz.py) hold the matches they claim, and the oracle
equals the reference on these very tiles.

* claims: at every seek distance (6, 10, 11, 12, 14; the bonus tiles at 10 and 14) the oracle's match
  list, rebuilt from its four streams, equals the reference's rule applied to the designed spans
  and backs alone (so nothing pasted from beyond the window by a back that is no whole number of
  rows appears), and holds every single-source paste as (p, min(L, 259), b) with its follow-ups;
* the oracle against the reference where it was built: find_lz's bytes and nuke map per design and
  distance, encode_tile's bytes per design and speed."""
import numpy as np
import pytest

import designed_lz as D
import oracle as O

KEYS = sorted(D.designs())
IDS = ["%s-%s" % k for k in KEYS]
needs_ref = pytest.mark.skipif(O.ref() is None, reason="oracle/_ref not built (no /root/reference)")


@pytest.fixture(scope="module")
def lz():
    D.warm(D.oracle_lz, D.lz_jobs())
    return D.oracle_lz


def dists(t):
    return [D.SPEED_DIST[sp] for sp in D.speeds_of(t)]


def overlaps(got, p, L):
    return [m for m in got if m[0] < p + L and p < m[0] + m[1]]


def test_designs_are_what_they_say():
    ds = D.designs()
    for shape in ("256x256", "300x260"):
        t = ds[("sweep", shape)]
        assert [b for _, _, b in t.pastes] == list(D.SWEEP_BACKS)
        assert {L for _, L, _ in t.pastes} == set(D.SWEEP_LENGTHS)
        assert all(r in D.SWEEP_BACKS and r + 1 in D.SWEEP_BACKS and r + 2 in D.SWEEP_BACKS for r in D.RING_REACH)
        t = ds[("runs", shape)]
        a = [n for _, n, c in t.runs if tuple(c) == tuple(t.runs[0][2])]
        assert a == list(D.RUN_LENGTHS) and len(t.runs) > len(a)
        assert any(s % t.w == 0 for s, _, _ in t.runs) and any(s % t.w == t.w - 1 for s, _, _ in t.runs)
        t = ds[("gaps", shape)]
        ps = [p for p, _, _ in t.pastes]
        assert ps[0] == 255 and [q - p - 8 for p, q in zip(ps[:5], ps[1:6])] == [254, 255, 256, 509, 510]
        assert t.pastes[-1][0] + t.pastes[-1][1] == t.n
        for n in D.BONUS_COLOURS:
            t = ds[("bonus%d" % n, shape)]
            assert t.colours == n and len(set(t.px[:, 1].tolist())) == 1
            assert t.pastes[0][1] == D.threshold(n) == t.short[1] + 1
        t = ds[("vertical", shape)]
        assert all(b % t.w == 0 for _, _, b in t.pastes[:-2]) and [b % t.w for _, _, b in t.pastes[-2:]] == [t.w - 1, 1]
    assert [D.threshold(n) for n in (33, 32, 16, 8, 4)] == [4, 6, 14, 24, 36]
    assert ds[("vertical", "256x300")].pastes[0][2] == 65536                  # 256 rows up: written as 0 / 0
    for shape in ("64x511", "140x400"):
        t = ds[("vertical", shape)]
        assert sum(b // t.w > 256 and b % t.w == 0 for _, _, b in t.pastes) == 3
    spans = ds[("stitch", "256x256")].spans
    assert all(any(s + 100 == X and L == 600 for s, L in spans) for X in D.SEG_STARTS)
    e = ds[("stitch-edges", "256x256")].pastes
    assert e[0][0] == D.SEG_STARTS[0] and e[1][0] + e[1][1] == D.SEG_STARTS[1] and e[2][:2] == (D.SEG_STARTS[2], 263)
    for k in (9, 70):
        t = ds[("rowperiod%d" % k, "256x256")]
        assert np.array_equal(t.px[k * 256:], t.px[:-k * 256])
        key = D.pack(t.px)
        same = np.flatnonzero(np.all([key[i:t.n - 3 + i] == key[D.DENSE_AT + i] for i in range(4)], axis=0))
        assert ((same >= D.DENSE_AT) & (same < D.DENSE_AT + 1024)).sum() > 64      # one posting group, the -s1 window


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_claims(lz, key):
    t = D.designs()[key]
    for dist in dists(t):
        got = D.oracle_matches(key, dist)
        assert D.encode_matches(got, t.n, dist) == lz(key, dist)[0], dist
        gs = set(got)
        want = D.expected(t, dist)
        if t.exact:
            assert got == want, (dist, [m for m in got if m not in set(want)][:4], [m for m in want if m not in gs][:4])
        assert all(m in gs for m in want), (dist, [m for m in want if m not in gs][:4])
        must, never = D.claims(t, dist)
        assert all(m in gs for m in must), (dist, [m for m in must if m not in gs][:4])
        for p, L, b in never:
            assert not overlaps(got, p, L), (dist, (p, L, b), overlaps(got, p, L))
        nuke = np.zeros(t.n, np.uint8)
        for p, L, _ in got:
            nuke[p:p + L] = 1
        assert np.array_equal(nuke, lz(key, dist)[1]), dist


@pytest.mark.parametrize("shape", ["256x256", "300x260"])
def test_claims_ties_and_caps(lz, shape):
    """the tie rules, literally"""
    t = D.designs()[("ties", shape)]
    for dist in D.DISTANCES:
        gs = set(D.oracle_matches(("ties", shape), dist))
        for name, (p, alts) in t.cases.items():
            (bf, Lf), (bn, Ln) = alts[0], alts[-1]                # farthest, nearest
            vis = [(b, L) for b, L in alts if D.visible(b, t.w, dist)]
            if not vis:
                assert not overlaps(gs, p, Lf), (dist, name)
            elif name.startswith("near") or name.startswith("cap"):
                b = min(b for b, _ in vis)                        # equal lengths: the nearest wins
                assert (p, min(Lf, 259), b) in gs, (dist, name)
                if Lf > 259:
                    assert (p + 259, Lf - 259, b) in gs, (dist, name)
            else:
                b, L = max(vis, key=lambda a: a[1])               # the longer wins, however far
                assert (p, L, b) in gs, (dist, name)
    t = D.designs()[("vertical", shape)]
    for dist in D.DISTANCES:
        gs = set(D.oracle_matches(("vertical", shape), dist))
        assert t.tie_h in gs, dist                                # as long as the vertical one: horizontal wins
        p, L, b = t.tie_v
        assert ((p, L, b) if dist > 8 else (p, L - 1, 41)) in gs, dist


@pytest.mark.parametrize("shape", ["256x256", "300x260"])
def test_claims_runs_and_bonus(lz, shape):
    t = D.designs()[("runs", shape)]
    for dist in D.DISTANCES:
        got = D.oracle_matches(("runs", shape), dist)
        own = [m for m in got if m[2] == 1]
        assert len(own) >= 10 and any(m[1] == 259 for m in own), dist
        if dist > 8:                                              # earlier runs in reach
            pairs = [(a, b) for a, b in zip(got, got[1:]) if a[2] > 1 and b[2] == 1 and b[0] == a[0] + a[1]]
            assert pairs and any(a[1] == 259 and a[2] > 1 for a in got), dist     # cross-run then own-run; a capped cross-run
    for n in D.BONUS_COLOURS:
        t = D.designs()[("bonus%d" % n, shape)]
        for dist in dists(t):
            got = D.oracle_matches((t.name, shape), dist)
            p, L, b = t.pastes[0]
            assert (p, L, b) in got and L == D.threshold(n), (n, dist)
            assert not overlaps(got, *t.short[:2]), (n, dist)     # a pixel shorter: nothing


def test_tiles_are_reproducible():
    """every design's file exists at every speed it runs at (OR_E_UNREPRODUCIBLE nowhere)"""
    out = D.warm(D.oracle_tile, D.tile_jobs())
    bad = [job for job, r in zip(D.tile_jobs(), out) if not isinstance(r, bytes)]
    assert not bad, bad


def _ref_lz(key, dist):
    t = D.designs()[key]
    return D.find_lz(O.ref().ref_find_lz_rgb, t.px, t.w, t.h, dist, D.threshold(t.colours) - 4)


def _ref_tile(key, speed):
    img = np.ascontiguousarray(D.designs()[key].image())
    out = np.empty(img.size * 8 + 65536, np.uint8)
    r = O.ref().ref_encode_tile(img.ctypes.data_as(O.u8p), img.shape[1], img.shape[0], speed, out.ctypes.data_as(O.u8p))
    return out[:r].tobytes()


@needs_ref
def test_oracle_equals_reference_find_lz(lz):
    jobs = D.lz_jobs()
    for (key, dist), (data, nuke) in zip(jobs, D.warm(_ref_lz, jobs)):
        mine = lz(key, dist)
        assert data == mine[0], (key, dist)
        assert np.array_equal(nuke, mine[1]), (key, dist)


@needs_ref
def test_oracle_equals_reference_encode_tile():
    jobs = D.tile_jobs()
    D.warm(D.oracle_tile, jobs)
    for (key, speed), data in zip(jobs, D.warm(_ref_tile, jobs)):
        assert data == D.oracle_tile(key, speed), (key, speed)
