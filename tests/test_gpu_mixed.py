"""GPU: mixed-shape batches of small images (hoh_encode_mixed_async / hoh_decode_mixed_async).

n images of n shapes go through one call: at -s0 one job on a staging surface, at -s1..-s4 the
uniform small stack per run of equal shapes.  Every file must be the bytes hoh_encode_image writes
for that image alone under HOH_OPT_SMALL_IMAGES, the recorded index the concatenation of the single
indexes, and the decode the input, with and without the index.  Single-image results are made once
per module and shared."""
import numpy as np
import pytest

from test_small_format import header

pytestmark = pytest.mark.gpu
E_ARG, E_CAP, E_UNSUPPORTED, E_CORRUPT = 1, 2, 6, 7

# every shape of A gives a sub-green tile (mode 128) for both noises, so it decodes; the shapes of T
# give palette tiles (mode 127, no palette): encode parity only
A = [(63, 65), (64, 64), (65, 63), (64, 48), (48, 300), (128, 129), (129, 128), (200, 100), (255, 255), (256, 256),
     (256, 200), (100, 256), (257, 130), (385, 300), (300, 511), (511, 300), (511, 16), (16, 511), (511, 1), (1, 511),
     (511, 511)]
T = [(1, 1), (2, 2), (7, 1), (1, 7), (3, 5)]


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
def mctx(hoh):
    """the context of the mixed calls: no option set"""
    c = hoh.Context(0)
    yield c
    c.close()


_IMG = {}


def synth_list(shapes):
    """synth_rgb(W, H, 7 + nz, nz), nz alternating 3 and 0 over the list"""
    from hoh_ans.synth import synth_rgb
    out = []
    for i, (W, H) in enumerate(shapes):
        nz = 0 if i % 2 else 3
        if (W, H, nz) not in _IMG:
            _IMG[(W, H, nz)] = synth_rgb(W, H, 7 + nz, nz)
        out.append(_IMG[(W, H, nz)])
    return out


_ONE = {}


def single(hoh, ctx, img, speed=0):
    """(file, index blob, Index) of one image through the synchronous call: made once, shared"""
    import torch
    key = (id(ctx), img.shape, img.tobytes(), speed)
    if key not in _ONE:
        H, W, _ = img.shape
        ix = hoh.Index()
        out, n, printed = hoh.encode_image(torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).cuda(), W, H, ctx=ctx,
                                           index=ix, speed=speed)
        torch.cuda.synchronize()
        assert n == printed
        _ONE[key] = (out[:n].cpu().numpy().tobytes(), ix.to_bytes(ctx), ix)
    return _ONE[key]


def shapes_of(imgs):
    return [(a.shape[1], a.shape[0]) for a in imgs]


def pack(torch, imgs):
    return torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in imgs])).cuda()


def mixed_encode(hoh, ctx, imgs, speed=0, index=None, stride=None):
    """one call into a 0xA5-filled buffer -> (out, stride, [(code, size)])"""
    import torch
    shapes = shapes_of(imgs)
    if stride is None:
        stride = max(hoh.lib().hoh_encode_bound(w, h) for w, h in shapes)
    out = torch.full((len(imgs) * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * len(imgs),), -1, dtype=torch.int64, device="cuda")
    hoh.encode_mixed_async(pack(torch, imgs), shapes, out, stride, st, ctx=ctx, index=index, speed=speed)
    torch.cuda.synchronize()
    return out, stride, [(int(a), int(b)) for a, b in st.cpu().numpy().reshape(-1, 2)]


def assert_files(hoh, out, stride, status, want):
    """file i and its status size are want[i]; the rest of its stride slot is still 0xA5"""
    for i, f in enumerate(want):
        assert status[i] == (0, len(f)), (i, status[i], len(f))
        slot = out[i * stride:(i + 1) * stride]
        assert slot[:len(f)].cpu().numpy().tobytes() == f, i
        assert bool((slot[len(f):] == 0xA5).all()), i


def mixed_decode(hoh, ctx, out, stride, shapes, index=None):
    """-> (packed output with 64 guard bytes behind it, all pre-filled with 0x5A; [(code, size)]; offsets)"""
    import torch
    total, off = hoh.mixed_rgb_bytes(shapes)
    dec = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * len(shapes),), -1, dtype=torch.int64, device="cuda")
    hoh.decode_mixed_async(out, stride, shapes, dec, st, ctx=ctx, index=index)
    torch.cuda.synchronize()
    return dec, [(int(a), int(b)) for a, b in st.cpu().numpy().reshape(-1, 2)], off


def assert_round_trip(hoh, ctx, out, stride, imgs, index=None, what=""):
    import torch
    shapes = shapes_of(imgs)
    dec, status, off = mixed_decode(hoh, ctx, out, stride, shapes, index)
    assert status == [(0, w * h * 3) for w, h in shapes], (what, status)
    assert torch.equal(dec[:off[-1]], pack(torch, imgs)), what
    assert bool((dec[off[-1]:] == 0x5A).all()), what               # the guard bytes behind the packed images


# ---------------------------------------------------------------- 1. encode parity at -s0

def test_parity_s0(hoh, orc, sctx, mctx):
    imgs = synth_list(A + T)
    want = [single(hoh, sctx, a)[0] for a in imgs]
    for k in range(4):
        W, H = A[k]
        assert want[k] == header(W, H) + orc.encode_tile(imgs[k], 0), k
    for a, f in zip(imgs[len(A):], want[len(A):]):
        assert f[len(header(a.shape[1], a.shape[0])) + 2] == 127       # the palette tiles of T
    out, stride, status = mixed_encode(hoh, mctx, imgs)
    assert_files(hoh, out, stride, status, want)
    out, stride, status = mixed_encode(hoh, mctx, imgs[::-1])
    assert_files(hoh, out, stride, status, want[::-1])
    # Wmax and Hmax from different images
    sub = synth_list([(511, 16), (16, 511), (64, 64)])
    out, stride, status = mixed_encode(hoh, mctx, sub)
    assert_files(hoh, out, stride, status, [single(hoh, sctx, a)[0] for a in sub])


# ---------------------------------------------------------------- 2. maxima of exactly 256 x 256

@pytest.mark.parametrize("order", [(0, 1, 2, 3), (1, 2, 3, 0)], ids=["256-first", "256-last"])
def test_front256_trap(hoh, sctx, mctx, order):
    """a batch whose maxima are 256 x 256 holds smaller tiles too: the front that takes w = h = 256
    for every tile must not run"""
    base = synth_list([(256, 256), (100, 256), (256, 100), (64, 64)])
    imgs = [base[k] for k in order]
    ix = hoh.Index()
    out, stride, status = mixed_encode(hoh, mctx, imgs, index=ix)
    assert_files(hoh, out, stride, status, [single(hoh, sctx, a)[0] for a in imgs])
    assert_round_trip(hoh, mctx, out, stride, imgs, ix, "index")
    assert_round_trip(hoh, mctx, out, stride, imgs, None, "no index")


# ---------------------------------------------------------------- 3. round trip of A

def test_round_trip(hoh, sctx, mctx):
    imgs = synth_list(A)
    ix = hoh.Index()
    out, stride, status = mixed_encode(hoh, mctx, imgs, index=ix)
    ones = [single(hoh, sctx, a) for a in imgs]
    assert_files(hoh, out, stride, status, [o[0] for o in ones])
    assert_round_trip(hoh, mctx, out, stride, imgs, ix, "recorded index")
    ctx = hoh.Context(0)
    for noix in (hoh.NOIX_ADAPTIVE, hoh.NOIX_LANES, hoh.NOIX_MULTI):
        ctx.set_option(hoh.OPT_NOIX_DECODER, noix)
        assert_round_trip(hoh, ctx, out, stride, imgs, hoh.Index(), "empty index, noix %d" % noix)
    ctx.close()
    cat = hoh.Index.concat([o[2] for o in ones], stride)
    blob = ix.to_bytes(mctx)
    assert len(blob) > 48 and cat.to_bytes() == blob
    assert_round_trip(hoh, mctx, out, stride, imgs, cat, "concatenated index")
    assert_round_trip(hoh, mctx, out, stride, imgs, hoh.Index.from_bytes(blob), "loaded index")


# ---------------------------------------------------------------- 4. a 256-wide tile beside wider ones

def test_flat_256(hoh, sctx, mctx):
    """Wmax > 256: the 256-wide tiles without copies take the flat plane layout, not the blocked one"""
    imgs = synth_list([(300, 260), (256, 200), (256, 256)])
    ix = hoh.Index()
    out, stride, status = mixed_encode(hoh, mctx, imgs, index=ix)
    assert_files(hoh, out, stride, status, [single(hoh, sctx, a)[0] for a in imgs])
    assert_round_trip(hoh, mctx, out, stride, imgs, ix, "index")
    assert_round_trip(hoh, mctx, out, stride, imgs, None, "no index")


# ---------------------------------------------------------------- 5. chain and LZ tiles

def natural_crop(W, H):
    """a W x H window of a natural image with more than 256 colours (fewer could give a palette tile,
    which no decoder reads): the first one on a coarse grid"""
    from hoh_ans.natural import natural_rgb
    if "nat" not in _IMG:
        _IMG["nat"] = natural_rgb(511, 511, 3)
    big = _IMG["nat"]
    for y in range(0, 511 - H + 1, 61):
        for x in range(0, 511 - W + 1, 67):
            c = np.ascontiguousarray(big[y:y + H, x:x + W])
            p = c.reshape(-1, 3).astype(np.uint32)
            if np.unique(p[:, 0] | p[:, 1] << 8 | p[:, 2] << 16).size > 256:
                return c
    raise AssertionError("no crop of %dx%d with more than 256 colours" % (W, H))


def test_lz_tiles(hoh, sctx, mctx):
    """designed LZ tiles of four shapes and natural crops: tiles in both width classes of the chain
    decoder, the second class with widths that are (64, 48) and are not (300, 140) multiples of 16"""
    import designed_lz as D
    by_shape = {}
    for (name, shape), t in D.designs().items():
        if 0 in D.speeds_of(t):
            by_shape.setdefault(shape, []).append(t)
    imgs = []
    for shape in ("256x256", "300x260", "64x511", "140x400"):
        assert by_shape.get(shape), shape
        imgs += [np.ascontiguousarray(t.image()) for t in by_shape[shape][:3]]
    imgs += [natural_crop(224, 224), natural_crop(511, 300), natural_crop(64, 48), natural_crop(48, 64)]
    ones = [single(hoh, sctx, a) for a in imgs]
    for a, o in zip(imgs, ones):
        assert o[0][len(header(a.shape[1], a.shape[0])) + 2] == 128
    for order in (list(range(len(imgs))), list(range(len(imgs)))[::-1]):
        sub = [imgs[k] for k in order]
        ix = hoh.Index()
        out, stride, status = mixed_encode(hoh, mctx, sub, index=ix)
        assert_files(hoh, out, stride, status, [ones[k][0] for k in order])
        assert_round_trip(hoh, mctx, out, stride, sub, ix, "index")
        assert_round_trip(hoh, mctx, out, stride, sub, None, "no index")


# ---------------------------------------------------------------- 6. speeds and decodable

SPEED_SHAPES = [(200, 100), (200, 100), (250, 250), (100, 41), (200, 100)]   # a run of two, a run of one, a shape seen before


def speed_images():
    from hoh_ans.synth import synth_rgb
    return [synth_rgb(W, H, 31 + i, 3) for i, (W, H) in enumerate(SPEED_SHAPES)]


@pytest.mark.parametrize("speed", [1, 2, 3, 4])
def test_speeds_decodable(hoh, dctx, speed):
    import torch
    imgs = speed_images()
    ctx = hoh.Context(0)
    ctx.set_option(hoh.OPT_DECODABLE, 1)
    ix = hoh.Index()
    hoh.encode_image(torch.from_numpy(imgs[0].reshape(-1)).cuda(), 200, 100, ctx=dctx, index=ix)   # not empty now
    assert len(ix.to_bytes(dctx)) > 48
    out, stride, status = mixed_encode(hoh, ctx, imgs, speed=speed, index=ix)
    assert_files(hoh, out, stride, status, [single(hoh, dctx, a, speed)[0] for a in imgs])
    assert len(ix.to_bytes(ctx)) == 48                             # emptied, as in the other -s>=1 calls
    assert_round_trip(hoh, ctx, out, stride, imgs, ix, "the emptied index")
    assert_round_trip(hoh, ctx, out, stride, imgs, None, "no index")
    ctx.close()


def test_speed1_jobs_in_flight(hoh, dctx):
    """natural images of six shapes at -s1: six jobs whose search takes milliseconds each, so the
    host enqueues job k + 1 (and rebuilds the search's per-shape log2 tables) while job k runs"""
    from hoh_ans.natural import natural_rgb
    imgs = [natural_rgb(W, H, 40 + i) for i, (W, H) in enumerate([(230, 250), (260, 200), (200, 260), (250, 230), (210, 240),
                                                                    (240, 210)])]
    ctx = hoh.Context(0)
    ctx.set_option(hoh.OPT_DECODABLE, 1)
    for _ in range(2):
        out, stride, status = mixed_encode(hoh, ctx, imgs, speed=1)
        assert_files(hoh, out, stride, status, [single(hoh, dctx, a, 1)[0] for a in imgs])
    assert_round_trip(hoh, ctx, out, stride, imgs, None, "no index")
    ctx.close()


def test_speed2_reference_bytes(hoh, sctx, mctx):
    imgs = speed_images()
    out, stride, status = mixed_encode(hoh, mctx, imgs, speed=2)
    assert_files(hoh, out, stride, status, [single(hoh, sctx, a, 2)[0] for a in imgs])


# ---------------------------------------------------------------- 7. one shape: the uniform batch

def test_uniform_equivalence(hoh, sctx, mctx):
    import torch
    from hoh_ans.natural import natural_rgb
    W = H = 224
    n = 8
    big = natural_rgb(W, H * n, 9)
    imgs = [big[i * H:(i + 1) * H] for i in range(n)]
    stride = hoh.lib().hoh_encode_bound(W, H)
    ref = torch.full((n * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
    ix0 = hoh.Index()
    hoh.encode_images_async(pack(torch, imgs), n, W, H, ref, stride, st, ctx=sctx, index=ix0)
    torch.cuda.synchronize()
    ix = hoh.Index()
    out, stride2, status = mixed_encode(hoh, mctx, imgs, index=ix)
    assert stride2 == stride
    assert status == [(int(a), int(b)) for a, b in st.cpu().numpy().reshape(-1, 2)]
    assert torch.equal(out, ref)
    assert ix.to_bytes(mctx) == ix0.to_bytes(sctx)
    assert_round_trip(hoh, mctx, out, stride, imgs, ix0, "the uniform batch's index")


# ---------------------------------------------------------------- 8. errors

def test_argument_errors(hoh, mctx):
    import torch
    rgb = torch.zeros(3 * 64 * 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(257 * 64, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2 * 257, dtype=torch.int64, device="cuda")
    cases = [([], E_ARG), ([(1, 1)] * 257, E_ARG), ([(8, 8), (0, 8)], E_ARG), ([(8, 8), (8, -3)], E_ARG),
             ([(8, 8), (512, 10)], E_UNSUPPORTED), ([(10, 512)], E_UNSUPPORTED)]
    for shapes, want in cases:
        with pytest.raises(hoh.HohError) as e:
            hoh.encode_mixed_async(rgb, shapes, out, 64, st, ctx=mctx)
        assert e.value.code == want, shapes
        with pytest.raises(hoh.HohError) as e:
            hoh.decode_mixed_async(out, 64, shapes, rgb, st, ctx=mctx)
        assert e.value.code == want, shapes
    with pytest.raises(hoh.HohError) as e:
        hoh.encode_mixed_async(rgb, [(8, 8)], out, 64, st, ctx=mctx, speed=5)
    assert e.value.code == E_ARG
    # null pointers, straight at the C ABI
    import ctypes as C
    wh = (C.c_int32 * 2)(8, 8)
    L, p = hoh.lib(), hoh.vp
    r, o, s = p(rgb.data_ptr()), p(out.data_ptr()), p(st.data_ptr())
    for args in ((None, wh, 0, o, 64, None, s, None), (r, None, 0, o, 64, None, s, None), (r, wh, 0, None, 64, None, s, None),
                 (r, wh, 0, o, 64, None, None, None), (r, wh, 0, o, 0, None, s, None)):
        assert L.hoh_encode_mixed_async(mctx.h, 1, *args) == E_ARG
    for args in ((None, 64, wh, r, None, s, None), (o, 64, None, r, None, s, None), (o, 64, wh, None, None, s, None),
                 (o, 64, wh, r, None, None, None), (o, 0, wh, r, None, s, None)):
        assert L.hoh_decode_mixed_async(mctx.h, 1, *args) == E_ARG
    assert L.hoh_encode_mixed_async(None, 1, r, wh, 0, o, 64, None, s, None) == E_ARG


def test_per_image_cap(hoh, sctx, mctx):
    """an image's own failure marks its slot only: a stride too small for image 1's file"""
    from hoh_ans.synth import synth_rgb
    imgs = [synth_rgb(100, 37, 3, 2), synth_rgb(120, 37, 4, 60), synth_rgb(100, 40, 5, 2)]
    files = [single(hoh, sctx, a)[0] for a in imgs]
    stride = max(len(files[0]), len(files[2])) + 8
    assert len(files[1]) > stride
    out, _, status = mixed_encode(hoh, mctx, imgs, stride=stride)
    assert [c for c, _ in status] == [0, E_CAP, 0]
    assert status[1][1] == len(files[1])                           # the size it would need
    for k in (0, 2):
        assert status[k][1] == len(files[k])
        assert out[k * stride:k * stride + len(files[k])].cpu().numpy().tobytes() == files[k]


def test_decode_errors(hoh, mctx):
    import torch
    imgs = synth_list([(200, 100), (64, 64), (100, 200), (129, 128)])
    shapes = shapes_of(imgs)
    ix = hoh.Index()
    out, stride, status = mixed_encode(hoh, mctx, imgs, index=ix)
    sizes = [s for _, s in status]
    assert all(c == 0 for c, _ in status)
    n = len(imgs)

    def refused(buf, shp, index=None):
        dec, st, off = mixed_decode(hoh, mctx, buf, stride, shp, index)
        assert st == [(E_CORRUPT, 0)] * n, st                       # every slot
        assert bool((dec == 0x5A).all())                            # the pre-filled output is untouched

    # two files' shapes swapped in h_wh: the header check on the device
    swapped = [shapes[2], shapes[1], shapes[0], shapes[3]]
    assert hoh.mixed_rgb_bytes(swapped)[0] == hoh.mixed_rgb_bytes(shapes)[0]
    refused(out, swapped)
    refused(out, swapped, ix)
    # one file truncated: its tail zeroed within its stride
    cut = out.clone()
    cut[2 * stride + sizes[2] // 2:3 * stride] = 0
    refused(cut, shapes)
    refused(cut, shapes, ix)
    # a file that stops right behind its header
    cut = out.clone()
    cut[stride + len(header(*shapes[1])):2 * stride] = 0xFF
    dec, st, _ = mixed_decode(hoh, mctx, cut, stride, shapes)
    assert all(c in (E_CORRUPT, E_UNSUPPORTED) for c, _ in st) and len({c for c, _ in st}) == 1
    assert bool((dec == 0x5A).all())
    # an index recorded for another stride or another n
    for (buf_stride, shp) in ((stride - 16, shapes), (stride, shapes[:3])):
        dec = torch.zeros(hoh.mixed_rgb_bytes(shp)[0], dtype=torch.uint8, device="cuda")
        st = torch.zeros(2 * len(shp), dtype=torch.int64, device="cuda")
        with pytest.raises(hoh.HohError) as e:
            hoh.decode_mixed_async(out, buf_stride, shp, dec, st, ctx=mctx, index=ix)
        assert e.value.code == E_ARG
    # the intact batch still decodes
    assert_round_trip(hoh, mctx, out, stride, imgs, ix, "after the refusals")


# ---------------------------------------------------------------- 9. allocation

def test_no_allocation_on_repeat(hoh):
    """grow-only workspaces: the same n, Wmax and Hmax allocate nothing, whatever the order"""
    import torch
    imgs = synth_list(A)
    order = np.random.RandomState(4).permutation(len(imgs))
    assert list(order) != sorted(order)
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


# ---------------------------------------------------------------- 10. the conveniences

def test_choh_dhoh_mixed(hoh, sctx, dctx, mctx):
    imgs = synth_list([(200, 100), (63, 65), (129, 128)])
    files = hoh.choh_mixed(imgs, ctx=mctx)
    assert files == [single(hoh, sctx, a)[0] for a in imgs]
    back = hoh.dhoh_mixed(files, shapes_of(imgs), ctx=mctx)
    assert all(np.array_equal(a, b) for a, b in zip(imgs, back))
    files = hoh.choh_mixed(imgs, ctx=mctx, speed=1, decodable=True)
    assert files == [single(hoh, dctx, a, 1)[0] for a in imgs]
    back = hoh.dhoh_mixed(files, shapes_of(imgs), ctx=mctx)
    assert all(np.array_equal(a, b) for a, b in zip(imgs, back))
