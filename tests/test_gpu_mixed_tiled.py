"""GPU: mixed-shape batches with tiled images (hoh_encode_mixed_async / hoh_decode_mixed_async).

Tiled shapes (any side of 512 or more) beside images of the small class, any order, one call: at -s0
one job over the tiles of all files (a tile table on the device, a vertically packed staging
surface), at -s1..-s4 the uniform batch per run of equal shapes.  Every file must be the bytes
hoh_encode_image writes for that image alone (a plain context for tiled shapes, an OPT_SMALL_IMAGES
one for small ones), the decode the packed input with and without the index, and file i's index out
of the batch's the blob of the image alone.  Single-image results are made once per module."""
import struct

import numpy as np
import pytest

from test_gpu_mixed import (assert_files, assert_round_trip, mixed_decode, mixed_encode, pack, shapes_of, single)

pytestmark = pytest.mark.gpu
E_ARG, E_CAP, E_UNSUPPORTED, E_CORRUPT = 1, 2, 6, 7

# (512,256) 2 tiles of 256^2 | (256,512) 1 x 2 | (513,257) tw 257, edge column 256 | (600,300) tw 300,
# no multiple of 16 | (1023,256) 3 columns of 341 | (520,770) 2 x 3, th 257, last row 256 | (300,512)
# one column, two rows | (511,1000) tw 511 | three of the small class
M = [(512, 256), (256, 512), (513, 257), (600, 300), (1023, 256), (520, 770), (300, 512), (511, 1000), (224, 224),
     (511, 511), (64, 48)]


def tiled(W, H):
    return (W >= 512 or H >= 512) and W >= 256 and H >= 256


@pytest.fixture(scope="module")
def hoh():
    import torch  # noqa: F401  (before the first context: torch brings its own HIP runtime)
    import hoh_ans
    return hoh_ans


def _ctx(hoh, small=0, decodable=0):
    c = hoh.Context(0)
    if small:
        c.set_option(hoh.OPT_SMALL_IMAGES, 1)
    if decodable:
        c.set_option(hoh.OPT_DECODABLE, 1)
    return c


@pytest.fixture(scope="module")
def ctxs(hoh):
    """plain / small: the single-image contexts; d*: the same with OPT_DECODABLE; mixed: no option"""
    cs = {"plain": _ctx(hoh), "small": _ctx(hoh, 1), "dplain": _ctx(hoh, 0, 1), "dsmall": _ctx(hoh, 1, 1),
          "mixed": _ctx(hoh), "dmixed": _ctx(hoh, 0, 1)}
    yield cs
    for c in cs.values():
        c.close()


_IMG = {}


def min_tile_colours(img):
    H, W, _ = img.shape
    xt, yt = (W // 256, H // 256) if tiled(W, H) else (1, 1)
    tw, th = -(-W // xt), -(-H // yt)
    p = img.astype(np.uint32)
    p = p[:, :, 0] | p[:, :, 1] << 8 | p[:, :, 2] << 16
    return min(np.unique(p[y:y + th, x:x + tw]).size for y in range(0, H, th) for x in range(0, W, tw))


def image(W, H, k):
    """k % 3: synth_rgb at noise 3, at noise 0, natural_rgb (LZ tiles).  A natural image takes the
    first seed from 11 on whose tiles all show more than 256 colours: fewer could give a palette
    tile, which no decoder reads."""
    from hoh_ans.natural import natural_rgb
    from hoh_ans.synth import synth_rgb
    key = (W, H, k % 3)
    if key not in _IMG:
        if k % 3 == 2:
            _IMG[key] = next(a for a in (natural_rgb(W, H, seed) for seed in range(11, 40)) if min_tile_colours(a) > 256)
        else:
            _IMG[key] = synth_rgb(W, H, 7 + 3 * (k % 3 == 0), 3 * (k % 3 == 0))
    return _IMG[key]


def images(shapes):
    return [image(W, H, k) for k, (W, H) in enumerate(shapes)]


def one(hoh, ctxs, img, speed=0, decodable=False):
    H, W, _ = img.shape
    name = ("d" if decodable else "") + ("plain" if tiled(W, H) else "small")
    return single(hoh, ctxs[name], img, speed)


# ---------------------------------------------------------------- 1. -s0 parity

@pytest.mark.parametrize("order", ["given", "shuffle1", "shuffle2"])
def test_parity_s0(hoh, ctxs, order):
    idx = list(range(len(M)))
    if order != "given":
        idx = list(np.random.RandomState(int(order[-1])).permutation(len(M)))
    imgs = [image(M[k][0], M[k][1], k) for k in idx]
    want = [one(hoh, ctxs, a)[0] for a in imgs]
    out, stride, status = mixed_encode(hoh, ctxs["mixed"], imgs)
    assert_files(hoh, out, stride, status, want)


# ---------------------------------------------------------------- 2. round trip

def test_round_trip(hoh, ctxs):
    imgs = images(M)
    total, off = hoh.mixed_rgb_bytes(M)
    assert sum(o % 4 != 0 for o in off[1:-1]) >= 3                 # neighbours share dwords
    ix = hoh.Index()
    out, stride, status = mixed_encode(hoh, ctxs["mixed"], imgs, index=ix)
    assert all(c == 0 for c, _ in status), status
    assert_round_trip(hoh, ctxs["mixed"], out, stride, imgs, ix, "recorded index")
    ctx = hoh.Context(0)
    for noix in (hoh.NOIX_ADAPTIVE, hoh.NOIX_LANES, hoh.NOIX_MULTI, hoh.NOIX_WAVE):
        ctx.set_option(hoh.OPT_NOIX_DECODER, noix)
        assert_round_trip(hoh, ctx, out, stride, imgs, None, "no index, noix %d" % noix)
    assert_round_trip(hoh, ctx, out, stride, imgs, hoh.Index(), "empty index")
    ctx.close()


# ---------------------------------------------------------------- 3. the side index

def test_index_per_file_and_joined(hoh, ctxs):
    imgs = images(M)
    mctx = ctxs["mixed"]
    ix = hoh.Index()
    out, stride, status = mixed_encode(hoh, mctx, imgs, index=ix)
    ones = [one(hoh, ctxs, a) for a in imgs]
    with pytest.raises(hoh.HohError) as e:                          # unequal tile counts: no version-1 blob
        ix.to_bytes(mctx)
    assert e.value.code == E_UNSUPPORTED
    assert ix.serialized_size() == 0
    blobs = [ix.file(i, mctx).to_bytes() for i in range(len(imgs))]
    for i, b in enumerate(blobs):
        assert len(b) > 48 and b == ones[i][1], i
    joined = hoh.Index.join([hoh.Index.from_bytes(b) for b in blobs], stride)
    with pytest.raises(hoh.HohError) as e:
        joined.to_bytes()
    assert e.value.code == E_UNSUPPORTED
    assert_round_trip(hoh, mctx, out, stride, imgs, joined, "joined index")
    assert joined.file(5).to_bytes() == blobs[5]
    # one checkpoint altered: the second one of file 5's (520 x 770, six tiles) tile 2, G plane
    blob = bytearray(blobs[5])
    nstreams = struct.unpack_from("<I", blob, 12)[0]
    assert nstreams == 7 * 6
    s, first = 2 * 7 + 3, 0
    for i in range(s):
        _, n, mode = struct.unpack_from("<QII", blob, 48 + 24 * i)
        first += (n + 255) // 256 if mode == 1 else 0
    _, n, mode = struct.unpack_from("<QII", blob, 48 + 24 * s)
    assert mode == 1 and n > 512
    blob[48 + 24 * nstreams + 12 * (first + 1)] ^= 1
    bad = hoh.Index.join([hoh.Index.from_bytes(bytes(blob) if i == 5 else b) for i, b in enumerate(blobs)], stride)
    dec, st, _ = mixed_decode(hoh, mctx, out, stride, M, bad)
    assert st == [(E_CORRUPT, 0)] * len(M), st
    assert bool((dec == 0x5A).all())
    # an empty index passes everywhere
    assert len(hoh.Index().file(3).to_bytes()) == 48
    assert len(hoh.Index.join([hoh.Index(), hoh.Index()], stride).to_bytes()) == 48


def test_index_equal_counts(hoh, ctxs):
    """equal tile counts serialise as before: concat of the singles, join the same bytes, and for a
    uniform tiled batch the blob and the files of hoh_encode_images_async"""
    import torch
    imgs = [image(512, 256, k) for k in range(3)]
    mctx = ctxs["mixed"]
    n, W, H = 3, 512, 256
    stride = hoh.lib().hoh_encode_bound(W, H)
    ref = torch.full((n * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
    ix0 = hoh.Index()
    hoh.encode_images_async(pack(torch, imgs), n, W, H, ref, stride, st, ctx=ctxs["plain"], index=ix0)
    torch.cuda.synchronize()
    ix = hoh.Index()
    out, stride2, status = mixed_encode(hoh, mctx, imgs, index=ix)
    assert stride2 == stride
    assert status == [(int(a), int(b)) for a, b in st.cpu().numpy().reshape(-1, 2)]
    assert torch.equal(out, ref)
    blob = ix.to_bytes(mctx)
    assert len(blob) > 48 and blob == ix0.to_bytes(ctxs["plain"])
    ones = [one(hoh, ctxs, a) for a in imgs]
    assert hoh.Index.concat([o[2] for o in ones], stride).to_bytes() == blob
    assert hoh.Index.join([o[2] for o in ones], stride).to_bytes() == blob
    assert [ix.file(i, mctx).to_bytes() for i in range(n)] == [o[1] for o in ones]
    # two tiles each in different grids ((512,256): 2 x 1, (256,512): 1 x 2): equal counts too
    imgs = [image(512, 256, 0), image(256, 512, 1)]
    ix = hoh.Index()
    out, stride, status = mixed_encode(hoh, mctx, imgs, index=ix)
    assert ix.to_bytes(mctx) == hoh.Index.concat([one(hoh, ctxs, a)[2] for a in imgs], stride).to_bytes()
    assert_round_trip(hoh, mctx, out, stride, imgs, hoh.Index.from_bytes(ix.to_bytes(mctx)), "loaded index")


# ---------------------------------------------------------------- 4. prefix sums over more than 64 / 128 files

def test_prefix_passes(hoh, ctxs):
    """256 images: the tile table's prefix sums (first tile, first row, packed offset) run over
    four waves; a 256^2-tile image beside a wider one (the flat layout for 256-wide tiles)"""
    shapes = [(64, 48)] * 256
    shapes[70] = (512, 256)
    shapes[200] = (600, 300)
    small = [image(64, 48, k) for k in range(3)]
    imgs = [small[k % 3] for k in range(256)]
    imgs[70] = image(512, 256, 0)
    imgs[200] = image(600, 300, 2)
    want = [one(hoh, ctxs, a)[0] for a in imgs]
    ix = hoh.Index()
    out, stride, status = mixed_encode(hoh, ctxs["mixed"], imgs, index=ix)
    assert_files(hoh, out, stride, status, want)
    assert_round_trip(hoh, ctxs["mixed"], out, stride, imgs, ix, "index")
    assert_round_trip(hoh, ctxs["mixed"], out, stride, imgs, None, "no index")
    assert ix.file(200, ctxs["mixed"]).to_bytes() == one(hoh, ctxs, imgs[200])[1]


# ---------------------------------------------------------------- 5. -s1 and -s4, plain and decodable

S_SHAPES = [(512, 256)] * 2 + [(600, 300)] + [(224, 224)] * 2


@pytest.mark.parametrize("decodable", [False, True], ids=["plain", "decodable"])
@pytest.mark.parametrize("speed", [1, 4])
def test_speeds(hoh, ctxs, speed, decodable):
    import torch
    from hoh_ans.synth import synth_rgb
    imgs = [synth_rgb(W, H, 31 + i, 3) for i, (W, H) in enumerate(S_SHAPES)]
    ctx = ctxs["dmixed" if decodable else "mixed"]
    ix = hoh.Index()
    hoh.encode_image(torch.from_numpy(imgs[0].reshape(-1)).cuda(), 512, 256, ctx=ctxs["plain"], index=ix)   # not empty now
    assert len(ix.to_bytes(ctxs["plain"])) > 48
    out, stride, status = mixed_encode(hoh, ctx, imgs, speed=speed, index=ix)
    assert_files(hoh, out, stride, status, [one(hoh, ctxs, a, speed, decodable)[0] for a in imgs])
    assert len(ix.to_bytes(ctx)) == 48                             # emptied, as in the other -s>=1 calls
    if decodable:
        assert_round_trip(hoh, ctx, out, stride, imgs, ix, "the emptied index")
        assert_round_trip(hoh, ctx, out, stride, imgs, None, "no index")


# ---------------------------------------------------------------- 6. errors

def test_decode_errors(hoh, ctxs):
    import torch
    from test_small_format import header
    shapes = [(512, 256), (64, 48), (256, 512), (520, 770)]
    imgs = images(shapes)
    mctx = ctxs["mixed"]
    ix = hoh.Index()
    out, stride, status = mixed_encode(hoh, mctx, imgs, index=ix)
    assert all(c == 0 for c, _ in status)
    n = len(imgs)

    def refused(buf, shp, index=None):
        dec, st, off = mixed_decode(hoh, mctx, buf, stride, shp, index)
        assert st == [(E_CORRUPT, 0)] * n, st                       # every slot
        assert bool((dec == 0x5A).all())                            # the pre-filled output is untouched

    # (512,256) and (256,512) swapped in h_wh (equal byte totals, equal tile counts)
    swapped = [shapes[2], shapes[1], shapes[0], shapes[3]]
    assert hoh.mixed_rgb_bytes(swapped)[0] == hoh.mixed_rgb_bytes(shapes)[0]
    refused(out, swapped)
    refused(out, swapped, ix)
    # a tiled file's xt - 1 byte
    hl = len(header(520, 770))
    bad = out.clone()
    assert int(bad[3 * stride + hl]) == 1 and int(bad[3 * stride + hl + 1]) == 2
    bad[3 * stride + hl] = 2
    refused(bad, shapes)
    refused(bad, shapes, ix)
    # its size table (five varints behind the tiling bytes) cut short: the slot's tail zeroed
    bad = out.clone()
    bad[3 * stride + hl + 2 + 4:4 * stride] = 0
    refused(bad, shapes)
    refused(bad, shapes, ix)
    # an index recorded for another stride or another n
    for (buf_stride, shp) in ((stride - 16, shapes), (stride, shapes[:3])):
        dec = torch.zeros(hoh.mixed_rgb_bytes(shp)[0], dtype=torch.uint8, device="cuda")
        st = torch.zeros(2 * len(shp), dtype=torch.int64, device="cuda")
        with pytest.raises(hoh.HohError) as e:
            hoh.decode_mixed_async(out, buf_stride, shp, dec, st, ctx=mctx, index=ix)
        assert e.value.code == E_ARG
    # the intact batch still decodes
    assert_round_trip(hoh, mctx, out, stride, imgs, ix, "after the refusals")
    assert_round_trip(hoh, mctx, out, stride, imgs, None, "after the refusals, no index")


def test_per_image_cap(hoh, ctxs):
    """a stride too small for the one tiled image: E_CAP in its slot only, with the size it needs"""
    from hoh_ans.synth import synth_rgb
    imgs = [synth_rgb(100, 37, 3, 2), synth_rgb(512, 256, 4, 60), synth_rgb(224, 224, 5, 2)]
    files = [one(hoh, ctxs, a)[0] for a in imgs]
    stride = max(len(files[0]), len(files[2])) + 8
    assert len(files[1]) > stride
    out, _, status = mixed_encode(hoh, ctxs["mixed"], imgs, stride=stride)
    assert [c for c, _ in status] == [0, E_CAP, 0]
    assert status[1][1] == len(files[1])
    for k in (0, 2):
        assert status[k][1] == len(files[k])
        assert out[k * stride:k * stride + len(files[k])].cpu().numpy().tobytes() == files[k]


# ---------------------------------------------------------------- 7. allocation

def test_no_allocation_on_repeat(hoh):
    import torch
    imgs = images(M)
    order = np.random.RandomState(4).permutation(len(imgs))
    ctx = hoh.Context(0)
    ix = hoh.Index()
    out, stride, status = mixed_encode(hoh, ctx, imgs, index=ix)
    assert_round_trip(hoh, ctx, out, stride, imgs, ix)
    assert_round_trip(hoh, ctx, out, stride, imgs, None)
    torch.cuda.synchronize()
    before = hoh.device_alloc_count()
    sub = [imgs[k] for k in order]
    out2, _, status2 = mixed_encode(hoh, ctx, sub, index=ix)
    assert hoh.device_alloc_count() == before
    assert_round_trip(hoh, ctx, out2, stride, sub, ix)
    assert_round_trip(hoh, ctx, out2, stride, sub, None)
    assert hoh.device_alloc_count() == before
    assert [s for _, s in status2] == [status[k][1] for k in order]
    ctx.close()


# ---------------------------------------------------------------- 8. the conveniences

def test_choh_dhoh_mixed(hoh, ctxs):
    shapes = [(63, 65), (600, 300), (256, 512), (129, 128)]
    imgs = images(shapes)
    files = hoh.choh_mixed(imgs, ctx=ctxs["mixed"])
    assert files == [one(hoh, ctxs, a)[0] for a in imgs]
    back = hoh.dhoh_mixed(files, shapes_of(imgs), ctx=ctxs["mixed"])
    assert all(np.array_equal(a, b) for a, b in zip(imgs, back))
    files = hoh.choh_mixed(imgs, ctx=ctxs["mixed"], speed=1, decodable=True)
    assert files == [one(hoh, ctxs, a, 1, True)[0] for a in imgs]
    back = hoh.dhoh_mixed(files, shapes_of(imgs), ctx=ctxs["mixed"])
    assert all(np.array_equal(a, b) for a, b in zip(imgs, back))
