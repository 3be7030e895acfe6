"""GPU: HOH_OPT_SMALL_IMAGES -- images of at most 511 x 511 as single-tile files, one or a batch.

The file of a small image is header || encode_tile(whole image): the bytes the reference's choh
codes and discards and its dhoh reads (dhoh.cpp:379); tests/test_small_format.py pins
that with the oracle alone.  Here the GPU's files are compared with the oracle's bytes, decoded by
the GPU through every entry point and by the oracle / tests/decodable_ref.py, and the batch calls
with the single-image ones.  Expected bytes and pixels are made once per module and shared."""
import os
import subprocess

import numpy as np
import pytest

import decodable_ref as dr
from test_small_format import decode_tile as or_decode_tile, header

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hoh-ans_amd", "bin")
E_ARG, E_CAP, E_UNSUPPORTED, E_CORRUPT = 1, 2, 6, 7

S0_SHAPES = [(63, 65), (64, 64), (65, 63), (200, 100), (255, 255), (256, 256), (385, 300), (300, 511), (511, 511)]
S0_CASES = [("synth", W, H, nz) for (W, H) in S0_SHAPES for nz in (3, 0)]
RT_CASES = S0_CASES + [("natural", 224, 224, 0), ("natural", 511, 300, 0)]
SPEED_CASES = [(W, H, sp) for (W, H) in ((200, 100), (250, 250)) for sp in (1, 2, 3, 4)]


def _id(c):
    return "%s-%dx%d-n%d" % c


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


_IMG = {}


def image(kind, W, H, nz):
    key = (kind, W, H, nz)
    if key not in _IMG:
        if kind == "synth":
            from hoh_ans.synth import synth_rgb
            _IMG[key] = synth_rgb(W, H, 7 + nz, nz)
        else:
            from hoh_ans.natural import natural_rgb
            _IMG[key] = natural_rgb(W, H, 3)
    return _IMG[key]


_ENC = {}


def encoded(hoh, sctx, case):
    """the GPU's -s0 file of a case with its recorded index's blob: encoded once, shared"""
    import torch
    if case not in _ENC:
        img = image(*case)
        H, W, _ = img.shape
        ix = hoh.Index()
        out, n, printed = hoh.encode_image(torch.from_numpy(img.reshape(-1)).cuda(), W, H, ctx=sctx, index=ix)
        torch.cuda.synchronize()
        _ENC[case] = (out[:n].cpu().numpy().tobytes(), printed, ix.to_bytes(sctx))
    return _ENC[case]


def _dev(torch, data, pad=0):
    return torch.from_numpy(np.frombuffer(bytes(data) + b"\0" * pad, np.uint8).copy()).cuda()


# ---------------------------------------------------------------- 1. option plumbing

def test_option_plumbing(hoh):
    import torch
    from hoh_ans.synth import synth_rgb
    ctx = hoh.Context(0)
    ctx.set_option(hoh.OPT_SMALL_IMAGES, 1)
    ctx.set_option(hoh.OPT_SMALL_IMAGES, 0)
    with pytest.raises(hoh.HohError) as e:
        ctx.set_option(hoh.OPT_SMALL_IMAGES, 2)
    assert e.value.code == E_ARG
    # at 0: the header-only file, and the enqueue-only and batched calls refuse the shape
    W, H = 300, 200
    img = synth_rgb(W, H, 3, 3)
    data, printed = hoh.choh(img, ctx=ctx)
    assert data == header(W, H) and len(data) == 10 and printed > 10
    rgb = torch.from_numpy(img.reshape(-1)).cuda()
    out = torch.zeros(2 * 4096, dtype=torch.uint8, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    two = torch.cat([rgb, rgb])
    for call in (lambda: hoh.encode_image_async(rgb, W, H, out, st, ctx=ctx),
                 lambda: hoh.decode_image_async(out, 4096, W, H, rgb.clone(), st, ctx=ctx),
                 lambda: hoh.encode_images_async(two, 2, W, H, out, 4096, st, ctx=ctx),
                 lambda: hoh.decode_images_async(out, 2, 4096, W, H, two.clone(), st, ctx=ctx)):
        with pytest.raises(hoh.HohError) as e:
            call()
        assert e.value.code == E_UNSUPPORTED
    with pytest.raises(hoh.HohError) as e:
        hoh.dhoh(data, ctx=ctx)
    assert e.value.code == E_UNSUPPORTED
    # at 1: untiled shapes outside the small class behave as at 0
    ctx.set_option(hoh.OPT_SMALL_IMAGES, 1)
    for (w, h) in ((600, 100), (100, 600)):
        wide = synth_rgb(w, h, 4, 3)
        d1, p1 = hoh.choh(wide, ctx=ctx)
        assert d1 == header(w, h) and p1 > len(d1)
        with pytest.raises(hoh.HohError) as e:
            hoh.dhoh(d1, ctx=ctx)
        assert e.value.code == E_UNSUPPORTED
        r1 = torch.from_numpy(wide.reshape(-1)).cuda()
        with pytest.raises(hoh.HohError) as e:
            hoh.encode_image_async(r1, w, h, out, st, ctx=ctx)
        assert e.value.code == E_UNSUPPORTED
        with pytest.raises(hoh.HohError) as e:
            hoh.encode_images_async(torch.cat([r1, r1]), 2, w, h, out, 4096, st, ctx=ctx)
        assert e.value.code == E_UNSUPPORTED
        with pytest.raises(hoh.HohError) as e:
            hoh.decode_images_async(out, 2, 4096, w, h, torch.cat([r1, r1]), st, ctx=ctx)
        assert e.value.code == E_UNSUPPORTED
    # ... and the small class gets its tile; choh(small=) sets the option for one call
    d2, p2 = hoh.choh(img, ctx=ctx)
    assert len(d2) == p2 == printed and d2[:10] == data
    ctx.set_option(hoh.OPT_SMALL_IMAGES, 0)
    assert hoh.choh(img, ctx=ctx, small=True) == (d2, p2)
    assert hoh.choh(img, ctx=ctx) == (data, printed)
    ctx.close()


# ---------------------------------------------------------------- 2. the reference's discarded bytes

@pytest.mark.parametrize("case", S0_CASES, ids=_id)
def test_parity_s0(hoh, orc, sctx, case):
    img = image(*case)
    H, W, _ = img.shape
    data, printed, _ = encoded(hoh, sctx, case)
    want = header(W, H) + orc.encode_tile(img, 0)
    assert printed == len(data) == orc.choh(img, 0)[1]
    assert data == want


@pytest.mark.parametrize("W,H,speed", SPEED_CASES, ids=["%dx%d-s%d" % c for c in SPEED_CASES])
def test_parity_speed(hoh, orc, sctx, W, H, speed):
    from hoh_ans.synth import synth_rgb
    img = synth_rgb(W, H, 11 + speed, 3)
    data, printed = hoh.choh(img, ctx=sctx, speed=speed)
    assert printed == len(data) == orc.choh(img, speed)[1]
    assert data == header(W, H) + orc.encode_tile(img, speed)


def test_parity_palette_2x2(hoh, orc, sctx):
    img = np.array([[[255, 0, 0], [0, 255, 0]], [[255, 255, 0], [0, 0, 255]]], np.uint8)
    data, printed = hoh.choh(img, ctx=sctx)
    tile = orc.encode_tile(img, 0)
    assert tile[2] == 127 and data == header(2, 2) + tile and printed == len(data) == orc.choh(img, 0)[1]
    with pytest.raises(hoh.HohError) as e:              # a palette tile carries no palette (Q15)
        hoh.dhoh(data, ctx=sctx)
    assert e.value.code == E_UNSUPPORTED


# ---------------------------------------------------------------- 3. round trip at -s0

@pytest.mark.parametrize("case", RT_CASES, ids=_id)
def test_round_trip_s0(hoh, orc, sctx, case):
    img = image(*case)
    H, W, _ = img.shape
    data, _, blob = encoded(hoh, sctx, case)
    assert data[len(header(W, H)) + 2] == 128            # sub-green
    r, back = or_decode_tile(orc, data, len(header(W, H)), W, H)
    assert r >= 0 and np.array_equal(back, img)
    ctx = hoh.Context(0)
    ctx.set_option(hoh.OPT_SMALL_IMAGES, 1)
    for noix in (hoh.NOIX_ADAPTIVE, hoh.NOIX_LANES, hoh.NOIX_MULTI, hoh.NOIX_WAVE):
        ctx.set_option(hoh.OPT_NOIX_DECODER, noix)
        assert np.array_equal(hoh.dhoh(data, ctx=ctx), img), noix
    assert np.array_equal(hoh.dhoh(data, ctx=ctx, index=hoh.Index.from_bytes(blob)), img)
    ctx.close()


# ---------------------------------------------------------------- 4. decodable round trip

D_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (17, 300), (300, 17), (63, 65), (224, 224)]
CONTENT = ["noise", "natural", "flat", "two", "grey"]


def content(kind, W, H):
    from hoh_ans.natural import natural_rgb
    from hoh_ans.synth import synth_rgb
    if kind == "noise":
        return synth_rgb(W, H, 21, 3)
    if kind == "natural":
        return natural_rgb(W, H, 5)
    if kind == "flat":
        return np.full((H, W, 3), (10, 200, 77), np.uint8)
    if kind == "two":
        img = np.full((H, W, 3), (10, 200, 77), np.uint8)
        img[(np.add.outer(np.arange(H), np.arange(W)) // 3) % 2 == 1] = (250, 3, 128)
        return img
    g = ((np.add.outer(np.arange(H) * 3, np.arange(W) * 5)) % 251).astype(np.uint8)    # non-binary grey
    return np.stack([g, g, g], -1)


@pytest.mark.parametrize("kind", CONTENT)
@pytest.mark.parametrize("W,H", D_SHAPES, ids=["%dx%d" % s for s in D_SHAPES])
def test_decodable_round_trip(hoh, dctx, W, H, kind):
    img = content(kind, W, H)
    hl = len(header(W, H))
    for speed in range(5):
        data, printed = hoh.choh(img, ctx=dctx, speed=speed)
        assert printed == len(data) and data[:hl] == header(W, H), speed
        assert np.array_equal(hoh.dhoh(data, ctx=dctx), img), speed
        back, t = dr.decode_tile(data, hl, len(data), W, H, img)
        assert np.array_equal(back, img) and t["mode"] in (128, 2), speed


@pytest.mark.parametrize("speed", [0, 1])
def test_decodable_round_trip_511(hoh, dctx, speed):
    img = image("natural", 511, 511, 0)
    data, printed = hoh.choh(img, ctx=dctx, speed=speed)
    assert printed == len(data)
    assert np.array_equal(hoh.dhoh(data, ctx=dctx), img)
    back, _ = dr.decode_tile(data, len(header(511, 511)), len(data), 511, 511, img)
    assert np.array_equal(back, img)


# ---------------------------------------------------------------- 5. a file the GPU did not write

def test_foreign_file(hoh, sctx):
    W, H = 100, 128
    rs = np.random.RandomState(5)
    img = image("natural", 224, 224, 0)[40:40 + H, 30:30 + W].copy()
    img[60:90] = img[20:50]                                   # copies further back than 255 pixels
    layers = [(5, 4, dr.MASKS[:4], rs.randint(0, 4, 20)), (1, 1, [0xffbf], [0]), (3, 3, [0xffbf, 0x0003], rs.randint(0, 2, 9))]
    tile = dr.build_tile(img, layers, lz_distance=12, pbs=(15, 14, 16))
    data = header(W, H) + tile
    back, t = dr.decode_tile(data, len(header(W, H)), len(data), W, H, img)    # the helper reads its own file
    assert np.array_equal(back, img) and t["nlz"] == 4 and t["layers"][0]["mapped"]
    assert np.array_equal(hoh.dhoh(data, ctx=sctx), img)
    # the same file at every byte alignment, other bytes behind it (a file picked out of a batch buffer
    # whose stride is odd): the prob_bits-16 stream is decoded by one lane, whose payload loads are
    # wave-uniform
    import torch
    for off in (1, 2, 3):
        buf = torch.from_numpy(np.frombuffer(b"\xff" * off + data + b"\xff" * 64, np.uint8).copy()).cuda()
        rgb, w, h = hoh.decode_image(buf[off:], len(data), ctx=sctx)
        torch.cuda.synchronize()
        assert (w, h) == (W, H) and np.array_equal(rgb.cpu().numpy().reshape(H, W, 3), img), off


# ---------------------------------------------------------------- 6. enqueue-only calls

def test_async(hoh, sctx):
    import torch
    case = ("natural", 224, 224, 0)
    img = image(*case)
    W = H = 224
    data, _, blob = encoded(hoh, sctx, case)
    rgb = torch.from_numpy(img.reshape(-1)).cuda()
    cap = hoh.lib().hoh_encode_bound(W, H)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    st = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    ix = hoh.Index()
    hoh.encode_image_async(rgb, W, H, out, st, ctx=sctx, index=ix)
    torch.cuda.synchronize()
    assert hoh.check_status(st.cpu().numpy(), "encode") == len(data)
    assert out[:len(data)].cpu().numpy().tobytes() == data
    assert ix.to_bytes(sctx) == blob
    for index in (None, ix):
        dec = torch.zeros(W * H * 3, dtype=torch.uint8, device="cuda")
        st.fill_(-1)
        hoh.decode_image_async(out, cap, W, H, dec, st, ctx=sctx, index=index)
        torch.cuda.synchronize()
        assert hoh.check_status(st.cpu().numpy(), "decode") == W * H * 3 and torch.equal(dec, rgb)
    # a wrong W or H: the header check fails on the device
    for (w, h) in ((223, 224), (224, 225)):
        dec = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
        st.fill_(-1)
        hoh.decode_image_async(out, cap, w, h, dec, st, ctx=sctx)
        torch.cuda.synchronize()
        assert int(st[0]) == E_CORRUPT, (w, h)
    # a cap below the file
    small = torch.zeros(len(data) - 1, dtype=torch.uint8, device="cuda")
    st.fill_(-1)
    hoh.encode_image_async(rgb, W, H, small, st, ctx=sctx)
    torch.cuda.synchronize()
    assert int(st[0]) == E_CAP


# ---------------------------------------------------------------- 7. batches

BATCHES = [(64, 64, 33, 0, 0), (100, 37, 33, 0, 0), (224, 224, 5, 0, 0), (511, 511, 2, 0, 0), (224, 224, 5, 2, 0),
           (224, 224, 5, 2, 1)]


@pytest.mark.parametrize("W,H,n,speed,decodable", BATCHES, ids=["%dx%dx%d-s%d-d%d" % b for b in BATCHES])
def test_batch(hoh, sctx, dctx, W, H, n, speed, decodable):
    import torch
    from hoh_ans.natural import natural_rgb
    from hoh_ans.synth import synth_rgb
    ctx = dctx if decodable else sctx
    img = W * H * 3
    if W * H < 40000:
        # noise: a natural crop this small can hold <= 256 colours and come out as a palette tile
        # (mode 127, Q15), which no decoder reads
        big = np.concatenate([synth_rgb(W, H, 100 + i, 3) for i in range(n)])
    else:
        big = natural_rgb(W, H * n, 9)                        # n different images: the rows of one tall one
    rgb = torch.from_numpy(big.reshape(-1)).cuda()
    stride = hoh.lib().hoh_encode_bound(W, H)
    out = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
    idx = hoh.Index()
    hoh.encode_images_async(rgb, n, W, H, out, stride, st, ctx=ctx, index=idx, speed=speed)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    singles, sizes = [], []
    for i in range(n):
        size = hoh.check_status(s[2 * i:2 * i + 2], "batch encode %d" % i)
        ix1 = hoh.Index()
        one, m, printed = hoh.encode_image(rgb[i * img:(i + 1) * img], W, H, ctx=ctx, index=ix1, speed=speed)
        torch.cuda.synchronize()
        assert size == m == printed and torch.equal(out[i * stride:i * stride + m], one[:m]), i
        singles.append(ix1)
        sizes.append(m)
    blob = idx.to_bytes(ctx)
    assert blob == hoh.Index.concat(singles, stride).to_bytes()
    assert (len(blob) > 48) == (speed == 0)                   # -s>=1: the empty index
    if speed and not decodable:
        return                                                # the reference's -s>=1 layers do not read back (Q14)
    for index in ((idx, None) if speed == 0 else (None,)):
        dec = torch.zeros(n * img, dtype=torch.uint8, device="cuda")
        ds = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
        hoh.decode_images_async(out, n, stride, W, H, dec, ds, ctx=ctx, index=index)
        torch.cuda.synchronize()
        d = ds.cpu().numpy()
        for i in range(n):
            assert hoh.check_status(d[2 * i:2 * i + 2], "batch decode %d" % i) == img
        assert torch.equal(dec, rgb), ("index" if index is not None else "no index")
    if (W, H, speed) != (224, 224, 0):
        return
    # a stride that cuts file 1 short (the largest file between two copies of the smallest): corrupt,
    # and never read on into file 2's bytes
    lo, hi = int(np.argmin(sizes)), int(np.argmax(sizes))
    tight = max(sizes[hi] - 40, sizes[lo])
    assert tight < sizes[hi]
    buf = torch.zeros(3 * tight, dtype=torch.uint8, device="cuda")
    for k, src in enumerate((lo, hi, lo)):
        m = min(sizes[src], tight)
        buf[k * tight:k * tight + m] = out[src * stride:src * stride + m]
    dec = torch.zeros(3 * img, dtype=torch.uint8, device="cuda")
    ds = torch.full((6,), -1, dtype=torch.int64, device="cuda")
    hoh.decode_images_async(buf, 3, tight, W, H, dec, ds, ctx=ctx)
    torch.cuda.synchronize()
    assert int(ds[2]) == E_CORRUPT


def test_batch_per_image_status(hoh, sctx):
    """an image's own failure marks its slot only: a stride too small for image 1's file"""
    import torch
    from hoh_ans.synth import synth_rgb
    W, H, n = 100, 37, 3
    img = W * H * 3
    imgs = [synth_rgb(W, H, 3, 2), synth_rgb(W, H, 4, 60), synth_rgb(W, H, 5, 2)]
    rgb = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).cuda()
    files = [hoh.choh(i, ctx=sctx)[0] for i in imgs]
    stride = max(len(files[0]), len(files[2])) + 8
    assert len(files[1]) > stride
    out = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
    hoh.encode_images_async(rgb, n, W, H, out, stride, st, ctx=sctx)
    torch.cuda.synchronize()
    codes = st.cpu().numpy().reshape(-1, 2)
    assert [int(c) for c in codes[:, 0]] == [0, E_CAP, 0]
    for k in (0, 2):
        assert out[k * stride:k * stride + len(files[k])].cpu().numpy().tobytes() == files[k]


# ---------------------------------------------------------------- 8. index from the file

@pytest.mark.parametrize("case", [("natural", 224, 224, 0), ("natural", 511, 300, 0)], ids=_id)
def test_index_build(hoh, sctx, case):
    import torch
    img = image(*case)
    data, _, blob = encoded(hoh, sctx, case)
    d = _dev(torch, data)
    built = hoh.build_index(d, len(data), ctx=sctx)
    assert built.to_bytes(sctx) == blob
    assert np.array_equal(hoh.dhoh(data, ctx=sctx, index=hoh.Index.from_bytes(blob)), img)
    ctx0 = hoh.Context(0)                                      # option off: untiled files are refused
    with pytest.raises(hoh.HohError) as e:
        hoh.build_index(d, len(data), ctx=ctx0)
    assert e.value.code == E_UNSUPPORTED
    ctx0.close()


# ---------------------------------------------------------------- 9. malformed input

def test_malformed(hoh, sctx):
    """error returns only: every parse is bounded by the size given"""
    import torch
    W = H = 224
    data, _, _ = encoded(hoh, sctx, ("natural", 224, 224, 0))
    hl = len(header(W, H))
    # the tile: 0 0 mode 0x03, then the first LZ stream: 2 varints, meta, table
    nested = bytearray(data)
    nested[hl] = 1
    cases = [("after the header", data[:hl], E_UNSUPPORTED), ("after the tiling bytes", data[:hl + 2], E_CORRUPT),
             ("mid-table", data[:hl + 9], E_CORRUPT), ("mid-payload", data[:len(data) // 2], E_CORRUPT),
             ("nested tiling", bytes(nested), E_UNSUPPORTED)]
    for name, bad, want in cases:
        with pytest.raises(hoh.HohError) as e:
            hoh.dhoh(bad, ctx=sctx)
        assert e.value.code == want, name
        d = _dev(torch, bad, pad=16)
        dec = torch.zeros(W * H * 3, dtype=torch.uint8, device="cuda")
        st = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        try:
            hoh.decode_image_async(d, len(bad), W, H, dec, st, ctx=sctx)
            torch.cuda.synchronize()
            code = int(st[0])
        except hoh.HohError as err:                          # refused before anything was enqueued
            code = err.code
        assert code == want, name


# ---------------------------------------------------------------- 10. allocation

def test_no_allocation_on_repeat(hoh):
    import torch
    from hoh_ans.natural import natural_rgb
    ctx = hoh.Context(0)
    ctx.set_option(hoh.OPT_SMALL_IMAGES, 1)
    W, H, n = 100, 37, 4
    img = W * H * 3
    rgb = torch.from_numpy(natural_rgb(W, H * n, 2).reshape(-1)).cuda()
    stride = hoh.lib().hoh_encode_bound(W, H)
    out = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    dec = torch.zeros(n * img, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    idx = hoh.Index()

    def once():
        hoh.encode_images_async(rgb, n, W, H, out, stride, st, ctx=ctx, index=idx)
        hoh.decode_images_async(out, n, stride, W, H, dec, st, ctx=ctx, index=idx)
        hoh.decode_images_async(out, n, stride, W, H, dec, st, ctx=ctx)
        f, m, _ = hoh.encode_image(rgb[:img], W, H, ctx=ctx)
        hoh.decode_image(f, m, out_dev=dec[:img], ctx=ctx)
        torch.cuda.synchronize()

    once()
    before = hoh.device_alloc_count()
    once()
    assert hoh.device_alloc_count() == before
    assert torch.equal(dec[:img], rgb[:img])
    ctx.close()


# ---------------------------------------------------------------- 11. command line

def test_cli(hoh, tmp_path):
    from hoh_ans.natural import natural_rgb
    W, H = 300, 200
    img = natural_rgb(W, H, 6)
    src, f, back = tmp_path / "in.rgb", tmp_path / "out.hoh", tmp_path / "back.rgb"
    src.write_bytes(img.tobytes())
    r = subprocess.run([os.path.join(BIN, "choh"), str(src), str(f), str(W), str(H), "-s0", "--small-images"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout.split()[-1]) == f.stat().st_size > 10
    r = subprocess.run([os.path.join(BIN, "dhoh"), str(f), str(back)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert back.read_bytes() == img.tobytes()
    # without the flag: the reference's header-only file, which dhoh refuses as before
    r = subprocess.run([os.path.join(BIN, "choh"), str(src), str(f), str(W), str(H), "-s0"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and f.stat().st_size == 10
    r = subprocess.run([os.path.join(BIN, "dhoh"), str(f), str(back)], capture_output=True, text=True, timeout=120)
    assert r.returncode == E_UNSUPPORTED
