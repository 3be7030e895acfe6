"""HOH_OPT_DECODABLE: -s0..-s4 files that read back.  The encoder is checked against the oracle
through tests/decodable_ref.py (independent of the GPU decoder), the GPU decoder against files it
did not write (the helper's builder), and both together by round trips through every entry point."""
import os
import subprocess

import numpy as np
import pytest

import decodable_ref as dr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hoh-ans_amd", "bin")
E_CORRUPT = 7


@pytest.fixture(scope="module")
def hoh():
    import torch  # noqa: F401  (before the first context: torch brings its own HIP runtime)
    import hoh_ans
    return hoh_ans


@pytest.fixture(scope="module")
def dctx(hoh):
    c = hoh.Context(0)
    c.set_option(hoh.OPT_DECODABLE, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def nat512():
    from hoh_ans.natural import natural_rgb
    return natural_rgb(512, 256, seed=3)


@pytest.fixture(scope="module")
def files512(hoh, dctx, nat512):
    """the 512x256 natural image at every speed, option on: encoded once, shared"""
    return {s: hoh.choh(nat512, ctx=dctx, speed=s)[0] for s in range(5)}


# ---------------------------------------------------------------- 1. option plumbing

def test_option_plumbing(hoh, nat512):
    ctx = hoh.Context(0)
    ctx.set_option(hoh.OPT_DECODABLE, 1)
    ctx.set_option(hoh.OPT_DECODABLE, 0)
    with pytest.raises(hoh.HohError):
        ctx.set_option(hoh.OPT_DECODABLE, 2)
    fresh = hoh.Context(0)
    assert hoh.choh(nat512, ctx=ctx, speed=2) == hoh.choh(nat512, ctx=fresh, speed=2)
    ctx.close()
    fresh.close()


# ---------------------------------------------------------------- 2. round trips

@pytest.mark.parametrize("speed", [0, 1, 2, 3, 4])
def test_round_trip_512x256(hoh, dctx, nat512, files512, speed):
    assert np.array_equal(hoh.dhoh(files512[speed], ctx=dctx), nat512)


@pytest.mark.parametrize("speed", [0, 1, 2, 3, 4])
def test_round_trip_700x520(hoh, speed):
    from hoh_ans.natural import natural_rgb
    img = natural_rgb(700, 520, seed=4)                       # 350 x 260 tiles: the non-256 path
    data, _ = hoh.choh(img, speed=speed, decodable=True)
    assert np.array_equal(hoh.dhoh(data), img)


@pytest.mark.parametrize("speed", [0, 1, 2, 3, 4])
def test_round_trip_batch_768x512(hoh, dctx, speed):
    import torch
    from hoh_ans.natural import natural_rgb
    W, H, n = 768, 512, 3
    imgs = np.stack([natural_rgb(W, H, seed=10 + i) for i in range(n)])
    rgb = torch.from_numpy(imgs.reshape(-1).copy()).cuda()
    stride = hoh.lib().hoh_encode_bound(W, H)
    out = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    dec = torch.zeros(n * W * H * 3, dtype=torch.uint8, device="cuda")
    st = torch.zeros(4 * n, dtype=torch.int64, device="cuda")
    hoh.encode_images_async(rgb, n, W, H, out, stride, st[:2 * n], ctx=dctx, speed=speed)
    hoh.decode_images_async(out, n, stride, W, H, dec, st[2 * n:], ctx=dctx)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    for i in range(2 * n):
        hoh.check_status(s[2 * i:2 * i + 2], "batch -s%d slot %d" % (speed, i))
    assert torch.equal(dec, rgb)


def test_round_trip_two_shards_s3(hoh, dctx):
    import torch
    from hoh_ans import dist as hd
    from hoh_ans.natural import natural_rgb
    W, H, world = 512, 512, 2
    img = natural_rgb(W, H, seed=6)
    L = hoh.lib()
    for r in range(world):
        t0, nt, y0, y1 = hd.shard(W, H, r, world)
        rows = y1 - y0
        rgb = torch.from_numpy(img[y0:y1].reshape(-1).copy()).cuda()
        out = torch.empty(L.hoh_encode_bound(W, rows), dtype=torch.uint8, device="cuda")
        sz = torch.empty(nt, dtype=torch.int32, device="cuda")
        n = hoh.encode_tiles(rgb, W, H, t0, nt, out, sz, ctx=dctx, row0=y0, speed=3)
        ts = sz.cpu().numpy().astype(np.uint32)
        dec = torch.zeros(W * rows * 3, dtype=torch.uint8, device="cuda")
        hoh.decode_tiles(out, n, W, H, t0, ts, dec, ctx=dctx, row0=y0)
        torch.cuda.synchronize()
        assert torch.equal(dec, rgb), "shard %d" % r


# ---------------------------------------------------------------- 3. the encoder against the oracle

@pytest.mark.parametrize("speed", [0, 1, 2, 3, 4])
def test_encoder_against_oracle(hoh, orc, nat512, files512, speed):
    data = files512[speed]
    back, tiles = dr.decode_file(data, nat512)
    assert np.array_equal(back, nat512)
    for t in tiles:
        for k, L in enumerate(t["layers"]):
            rng = 1 << (9 if (k and t["mode"] == 128) else 8)
            if speed == 0:                                     # today's layer: MED at prob_bits 15
                assert L["masks"] == [0x10] and not L["mapped"]
                assert L["stream"] == orc.encode_entropy(L["res"], rng, 15)
            else:
                pb, want = dr.ladder_pb(L["res"], rng)
                assert L["stream"] == want, (speed, k, pb, L["pb"])
    off, _ = hoh.choh(nat512, speed=speed, decodable=False)
    assert len(data) >= len(off)
    if speed == 0:
        assert data == off


# ---------------------------------------------------------------- 4. the decoder against foreign files

def _smooth(rs, W, H):
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(x * 2 + y) // 3, (x + y * 3) // 5, (x * y) // 97], -1) + rs.randint(-3, 4, (H, W, 3))
    return (img % 256).astype(np.uint8)


def test_decoder_foreign_files(hoh):
    rs = np.random.RandomState(17)
    W, H = 768, 256
    img = _smooth(rs, W, H)
    img[:, 512:] = rs.randint(0, 256, (H, 256, 3))            # a noise tile: its residual streams are stored
    img[30] = img[29]                                          # vertical copies of 1, 7 and 255 rows
    img[60:64] = img[53:57]
    img[255, :512] = img[0, :512]
    rects = dr.tile_rects(W, H)
    every = dr.MASKS + [0x5a3c]                                # the 14 stock masks and an arbitrary one
    specs = [
        # random maps over all masks on the 40-px grid, 4-stream LZ, prob_bits 12 / 16 / 19
        dict(layers=[(7, 7, every, rs.randint(0, 15, 49)) for _ in range(3)], lz=10, pbs=(12, 16, 19)),
        # a grid that is not 40 px, a single-mask map, a 1x1 map other than 0x0010; RGB mode; 3-stream LZ
        dict(layers=[(5, 9, dr.MASKS[4:9], rs.randint(0, 5, 45)), (3, 4, [0xffff], np.zeros(12, int)),
                     (1, 1, [0xffbf], [0])], lz=6, pbs=(15, 14, 13), mode=2),
        dict(layers=[(2, 2, [0x0010, 0x0001], rs.randint(0, 2, 4)) for _ in range(3)], lz=None, pbs=(15, 15, 15)),
    ]
    tiles = []
    for (x0, y0, w, h), sp in zip(rects, specs):
        tiles.append(dr.build_tile(img[y0:y0 + h, x0:x0 + w], sp["layers"], mode=sp.get("mode", 128),
                                   lz_distance=sp["lz"], pbs=sp["pbs"]))
    data = dr.build_file(W, H, tiles)
    back, parsed = dr.decode_file(data, img)                   # the helper reads its own file
    assert np.array_equal(back, img)
    assert [t["nlz"] for t in parsed] == [4, 3, 3] and [t["mode"] for t in parsed] == [128, 2, 128]
    assert [L["pb"] for L in parsed[0]["layers"]] == [12, 16, 19]
    assert all(L["pb"] is None for L in parsed[2]["layers"])   # stored
    backs = {m[2] // 256 for m in parsed[0]["matches"] if m[2] % 256 == 0}
    assert {1, 7, 255} <= backs, backs
    assert np.array_equal(hoh.dhoh(data), img)


# ---------------------------------------------------------------- 5. named corners

def test_corner_distance_65536(hoh, dctx):
    """each tile's row 256 repeats its row 0: the reference's LZ takes the copy at distance 65536,
    stored as 0 / 0; a decodable file stops at 65535"""
    rs = np.random.RandomState(23)
    img = rs.randint(0, 256, (514, 512, 3)).astype(np.uint8)
    img[256] = img[0]
    img[513] = img[257]
    data, _ = hoh.choh(img, ctx=dctx, speed=1)
    for x0, y0, w, h, s, e in dr.tiles_of(data)[2]:
        t = dr.parse_tile(data, s, e, w, h)
        assert all(m[2] != 0 for m in t["matches"])
    assert np.array_equal(hoh.dhoh(data, ctx=dctx), img)


def test_corner_rgb_mode(hoh, dctx):
    rs = np.random.RandomState(29)
    y, x = np.mgrid[0:256, 0:512]
    img = np.stack([(x // 2) % 256, rs.randint(0, 256, (256, 512)), (y + x // 4) % 256], -1).astype(np.uint8)
    data, _ = hoh.choh(img, ctx=dctx, speed=3)
    modes = [data[s + 2] for _, _, _, _, s, _ in dr.tiles_of(data)[2]]
    assert 2 in modes, modes
    assert np.array_equal(hoh.dhoh(data, ctx=dctx), img)


@pytest.mark.parametrize("colour", [(128, 128, 128), (40, 90, 200)])
def test_corner_flat_tile(hoh, dctx, colour):
    """a flat tile (bitimage mode 0 / indexed mode 127 without the option) is sub-green.  At mid
    grey every plane sits at the predictors' border value (half), every predictor is exact in
    every cell and the map holds a single mask; any other colour mispredicts along the tile's first
    row and column, where the search (the reference's, unchanged) picks other masks."""
    rs = np.random.RandomState(31)
    img = rs.randint(0, 256, (256, 512, 3)).astype(np.uint8)
    img[:, :256] = colour
    data, _ = hoh.choh(img, ctx=dctx, speed=2)
    x0, y0, w, h, s, e = dr.tiles_of(data)[2][0]
    t = dr.parse_tile(data, s, e, w, h)
    assert t["mode"] == 128
    assert all(L["mapped"] for L in t["layers"])
    if colour == (128, 128, 128):
        assert all(len(L["masks"]) == 1 for L in t["layers"])
    assert np.array_equal(hoh.dhoh(data, ctx=dctx), img)


@pytest.mark.parametrize("speed", [0, 2])
def test_corner_grey(hoh, dctx, speed):
    rs = np.random.RandomState(37)
    y, x = np.mgrid[0:256, 0:512]
    g = ((x + 2 * y) // 3 + rs.randint(-2, 3, (256, 512))) % 256
    img = np.stack([g, g, g], -1).astype(np.uint8)
    data, _ = hoh.choh(img, ctx=dctx, speed=speed)
    assert np.array_equal(hoh.dhoh(data, ctx=dctx), img)


# ---------------------------------------------------------------- 6. corrupt input

def test_corrupt_inputs(hoh, orc):
    rs = np.random.RandomState(41)
    W, H = 512, 256
    img = _smooth(rs, W, H)
    masks = dr.MASKS[:3]

    def build(pidx0):
        tiles = []
        for k, (x0, y0, w, h) in enumerate(dr.tile_rects(W, H)):
            layers = [(7, 7, masks, pidx0 if (k == 0 and i == 0) else rs.randint(0, 3, 49)) for i in range(3)]
            tiles.append(dr.build_tile(img[y0:y0 + h, x0:x0 + w], layers))
        return dr.build_file(W, H, tiles), tiles

    good, tiles = build(rs.randint(0, 3, 49))
    assert np.array_equal(hoh.dhoh(good), img)
    # cut inside the first map stream of the last tile (whose size no table entry states): 3 framing
    # bytes, 0x03, three empty LZ streams and 0x24, two varints, 4 header bytes, 3 masks, the stream
    assert tiles[1][3:14] == bytes([0x03]) + orc.encode_entropy(np.zeros(0, np.uint16), 256, 10) * 3 + bytes([0x24])
    _, p = dr.rd_varint(tiles[1], 14)
    _, p = dr.rd_varint(tiles[1], p)
    assert tiles[1][p:p + 4] == bytes([0x10, 6, 6, 3])
    cut = good[:len(good) - len(tiles[1]) + p + 4 + 6 + 6]
    with pytest.raises(hoh.HohError) as e:
        hoh.dhoh(cut)
    assert e.value.code == E_CORRUPT
    # a map index that is not below the mask count: the map stream coded over a range of 4
    bad_idx = rs.randint(0, 3, 49)
    bad_idx[20] = 3
    t0 = dr.build_tile(img[:, :256], [(7, 7, masks + [0xffff], bad_idx)] + [(7, 7, masks, rs.randint(0, 3, 49))] * 2)
    # ... then the fourth mask dropped from the header: count 3, list shortened by two bytes
    L1_pos = 4 + 9 + 1
    l1, p = dr.rd_varint(t0, L1_pos)
    l2, p = dr.rd_varint(t0, p)
    assert t0[p:p + 4] == bytes([0x10, 6, 6, 4])
    layer = bytes([0x10, 6, 6, 3]) + t0[p + 4:p + 10] + t0[p + 12:p + l1]
    t0b = t0[:L1_pos] + dr.wr_varint(len(layer)) + dr.wr_varint(l2) + layer + t0[p + l1:]
    bad = dr.build_file(W, H, [t0b, tiles[1]])
    with pytest.raises(hoh.HohError) as e:
        hoh.dhoh(bad)
    assert e.value.code == E_CORRUPT


# ---------------------------------------------------------------- 7. plane level

def _plane(rs, h, w, depth, copies):
    y, x = np.mgrid[0:h, 0:w]
    d = (((x * 3 + y * 2) // 3 + rs.randint(-3, 4, (h, w))) % (1 << depth)).astype(np.uint16).reshape(-1)
    br = np.zeros(w * h, np.uint16)
    if copies:
        for _ in range(12):
            i, L, b = int(rs.randint(1, w * h)), int(rs.randint(1, 40)), int(rs.randint(1, 300))
            for k in range(i, min(w * h, i + L)):
                if k >= b:
                    br[k] = b
        for k in np.nonzero(br)[0]:
            d[k] = d[k - br[k]]
    return d.reshape(h, w), br


@pytest.mark.parametrize("speed", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", [(30, 20), (100, 128)])
def test_plane_level_round_trip(hoh, dctx, speed, w, h):
    rs = np.random.RandomState(50 + speed)
    for depth, copies in [(8, False), (9, True)]:
        d, br = _plane(rs, h, w, depth, copies)
        nuke = (br != 0).astype(np.uint8).reshape(h, w) if copies else None
        layer = hoh.layer_encode(d, depth, nuke, ctx=dctx, speed=speed)
        back = hoh.layer_decode(layer, w, h, depth, backref=br if copies else None, ctx=dctx)
        assert np.array_equal(np.asarray(back).reshape(h, w), d), (w, h, depth, copies)


# ---------------------------------------------------------------- 8. CLI

def test_cli_decodable(tmp_path, nat512):
    src = tmp_path / "in.rgb"
    src.write_bytes(nat512.tobytes())
    r = subprocess.run([os.path.join(BIN, "choh"), str(src), str(tmp_path / "o.hoh"), "512", "256", "-s2",
                        "--decodable"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(BIN, "dhoh"), str(tmp_path / "o.hoh"), str(tmp_path / "back.rgb")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "back.rgb").read_bytes() == nat512.tobytes()
