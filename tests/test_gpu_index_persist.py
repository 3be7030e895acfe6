"""GPU: the side index beside the file -- hoh_index_serialize / _deserialize / _build / _concat.

An index built from a file's bytes alone must serialize to the bytes of the index the encoder
recorded for that file (the blob is canonical), a loaded index must drive the indexed decoder on a
context that never saw the encode, a wrong checkpoint must fail the decode closed, per-file indexes
must concatenate into the batch encoder's index, and the empty index must be accepted everywhere.

Shapes: A synthetic 768x512 (3x2 tiles of 256^2: blocked planes, whole segments), B synthetic
1000x600 (334x300 tiles: partial last segment, flat layout, unaligned payloads), C natural 768x512
(LZ copies in every tile: short LZ streams, stored / empty modes, compacted planes), D three
synthetic 512x256 images (they stack as a batch)."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED, E_CORRUPT = 1, 6, 7
SEG = 256


@pytest.fixture(scope="module")
def hoh():
    import hoh_ans
    return hoh_ans


def _image(name):
    from hoh_ans import natural, synth
    if name == "A":
        return synth.synth_rgb(768, 512, seed=21, noise=4)
    if name == "B":
        return synth.synth_rgb(1000, 600, seed=21, noise=4)
    if name == "A22":
        return synth.synth_rgb(768, 512, seed=22, noise=4)
    return natural.natural_rgb(768, 512, seed=1)


@pytest.fixture(scope="module")
def enc(hoh):
    """name -> (image, .hoh bytes on the device, size, blob of the encoder's index), each encoded
    once on one context (closed before the tests decode on others)"""
    import torch
    ctx = hoh.Context(0)
    out = {}
    for name in ("A", "B", "C", "A22"):
        img = _image(name)
        H, W, _ = img.shape
        ix = hoh.Index()
        f, n, _ = hoh.encode_image(torch.from_numpy(img.reshape(-1)).cuda(), W, H, ctx=ctx, index=ix)
        torch.cuda.synchronize()
        blob = ix.to_bytes(ctx)
        assert len(blob) == ix.serialized_size()
        out[name] = (img, f, n, blob)
    ctx.close()
    return out


def _parse(blob):
    magic, ver, seg, ns, nimg, r0, stride, nck, r1 = struct.unpack_from("<4sIIIIIQQQ", blob, 0)
    assert (magic, ver, seg, r0, r1) == (b"HOHX", 1, SEG, 0, 0)
    recs = [struct.unpack_from("<QIIII", blob, 48 + 24 * s) for s in range(ns)]
    assert len(blob) == 48 + 24 * ns + 12 * nck
    return ns, nimg, stride, nck, recs


@pytest.mark.parametrize("kernel", ["lanes", "multi"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_built_equals_recorded(hoh, enc, name, kernel):
    """both chain kernels of the builder (it picks one as a no-index decode does; pinned here)"""
    img, f, n, E = enc[name]
    ns, nimg, stride, nck, recs = _parse(E)
    tiles = (img.shape[1] // 256) * (img.shape[0] // 256)
    assert ns == 7 * tiles and nimg == 1 and stride == 0
    assert nck == sum((r[1] + SEG - 1) // SEG for r in recs if r[2] == 1) > 0
    assert all(r[2] == 0 for r in recs[6::7])                 # the indexed plane is not in a sub-green tile
    ctx = hoh.Context(0)
    ctx.set_option(hoh.OPT_NOIX_DECODER, hoh.NOIX_LANES if kernel == "lanes" else hoh.NOIX_MULTI)
    built = hoh.build_index(f, n, ctx=ctx)
    F = built.to_bytes(ctx)
    assert len(F) == built.serialized_size() == len(E)
    assert F == E
    ctx.close()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_roundtrip_on_another_context(hoh, enc, name):
    import torch
    img, f, n, E = enc[name]
    H, W, _ = img.shape
    ctx = hoh.Context(0)
    ix = hoh.Index.from_bytes(E)
    assert ix.to_bytes() == E
    rgb, w, h = hoh.decode_image(f, n, ctx=ctx, index=ix)
    torch.cuda.synchronize()
    assert (w, h) == (W, H) and np.array_equal(rgb.cpu().numpy().reshape(H, W, 3), img)
    out = torch.zeros(W * H * 3, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hoh.decode_image_async(f, n, W, H, out, st, ctx=ctx, index=ix)
    torch.cuda.synchronize()
    assert hoh.check_status(st.cpu().numpy(), "decode_image_async") == W * H * 3
    assert np.array_equal(out.cpu().numpy().reshape(H, W, 3), img)
    ctx.close()


def test_loaded_index_is_used_and_fails_closed(hoh, enc):
    """one bit of xl in a mid-stream checkpoint of a G plane: the blob still loads (its structure is
    intact), the segment that ends there no longer meets it, the decode is HOH_E_CORRUPT"""
    import torch
    img, f, n, E = enc["A"]
    H, W, _ = img.shape
    ns, _, _, nck, recs = _parse(E)
    g = 7 * 2 + 3                                             # G plane of the third tile
    assert recs[g][2] == 1 and recs[g][1] == 65536
    first = sum((r[1] + SEG - 1) // SEG for r in recs[:g] if r[2] == 1)
    pos = 48 + 24 * ns + 12 * (first + 100)                   # xl of its checkpoint 100
    bad = bytearray(E)
    bad[pos] ^= 0x10
    ctx = hoh.Context(0)
    ixb = hoh.Index.from_bytes(bytes(bad))
    with pytest.raises(hoh.HohError) as ei:
        hoh.decode_image(f, n, ctx=ctx, index=ixb)
    assert ei.value.code == E_CORRUPT
    torch.cuda.synchronize()
    rgb, _, _ = hoh.decode_image(f, n, ctx=ctx, index=hoh.Index.from_bytes(E))
    torch.cuda.synchronize()
    assert np.array_equal(rgb.cpu().numpy().reshape(H, W, 3), img)
    ctx.close()


def test_foreign_index_never_gives_wrong_pixels(hoh, enc):
    import torch
    img, f, n, _ = enc["A"]
    H, W, _ = img.shape
    ctx = hoh.Context(0)
    other = hoh.Index.from_bytes(enc["A22"][3])
    try:
        rgb, _, _ = hoh.decode_image(f, n, ctx=ctx, index=other)
        torch.cuda.synchronize()
        assert np.array_equal(rgb.cpu().numpy().reshape(H, W, 3), img)
    except hoh.HohError as e:
        assert e.code == E_CORRUPT
    ctx.close()


def _batch(hoh, ctx, W, H, seeds, speed):
    """n images, their batch encode with an Index -> (rgb, files, stride, index)"""
    import torch
    n, img = len(seeds), W * H * 3
    stride = hoh.lib().hoh_encode_bound(W, H)
    rgb = torch.empty(n * img, dtype=torch.uint8, device="cuda")
    for i, sd in enumerate(seeds):
        rgb[i * img:(i + 1) * img] = hoh.synth_rgb_dev(W, H, sd, 4, ctx=ctx)
    out = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix = hoh.Index()
    hoh.encode_images_async(rgb, n, W, H, out, stride, st, ctx=ctx, index=ix, speed=speed)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    sizes = [hoh.check_status(s[2 * i:2 * i + 2], "batch encode %d" % i) for i in range(n)]
    return rgb, out, stride, ix, sizes


def _decode_batch(hoh, ctx, out, n, stride, W, H, ix):
    import torch
    dec = torch.zeros(n * W * H * 3, dtype=torch.uint8, device="cuda")
    ds = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hoh.decode_images_async(out, n, stride, W, H, dec, ds, ctx=ctx, index=ix)
    torch.cuda.synchronize()
    d = ds.cpu().numpy()
    for i in range(n):
        assert hoh.check_status(d[2 * i:2 * i + 2], "batch decode %d" % i) == W * H * 3
    return dec


def test_concat_equals_batch_index(hoh, enc):
    import torch
    W, H, n = 512, 256, 3
    ctx = hoh.Context(0)
    rgb, out, stride, bix, sizes = _batch(hoh, ctx, W, H, [1, 2, 3], 0)
    want = bix.to_bytes(ctx)
    assert _parse(want)[1:3] == (n, stride)
    singles = []
    for i in range(n):                                        # each file's own index, through its blob
        one = hoh.build_index(out[i * stride:i * stride + sizes[i]].clone(), sizes[i], ctx=ctx)
        singles.append(hoh.Index.from_bytes(one.to_bytes(ctx)))
    cat = hoh.Index.concat(singles, stride)
    assert cat.to_bytes() == want
    ctx2 = hoh.Context(0)
    dec = _decode_batch(hoh, ctx2, out, n, stride, W, H, cat)
    assert torch.equal(dec, rgb)
    assert hoh.Index.concat(singles[:1], stride).to_bytes() == singles[0].to_bytes()   # n == 1 copies
    for bad in ([singles[0], hoh.Index.from_bytes(enc["A"][3])], [cat, cat]):           # nstreams differ; a batch index
        with pytest.raises(hoh.HohError) as ei:
            hoh.Index.concat(bad, stride)
        assert ei.value.code == E_ARG
    ctx.close()
    ctx2.close()


def test_unsupported_and_empty(hoh):
    import torch
    from hoh_ans import natural
    ctx = hoh.Context(0)
    ctx.set_option(hoh.OPT_DECODABLE, 1)
    img = natural.natural_rgb(512, 256, seed=3)
    f, n, _ = hoh.encode_image(torch.from_numpy(img.reshape(-1)).cuda(), 512, 256, ctx=ctx, speed=1)
    torch.cuda.synchronize()
    ix = hoh.Index()
    with pytest.raises(hoh.HohError) as ei:
        hoh.build_index(f, n, ctx=ctx, index=ix)
    assert ei.value.code == E_UNSUPPORTED
    assert ix.nbytes() == 0 and len(ix.to_bytes()) == 48
    assert hoh.Index.from_bytes(ix.to_bytes()).nbytes() == 0
    rgb, _, _ = hoh.decode_image(f, n, ctx=ctx, index=ix)
    torch.cuda.synchronize()
    assert np.array_equal(rgb.cpu().numpy().reshape(256, 512, 3), img)
    # the index a -s2 batch encode was given is empty, and a batched decode takes it: stacked
    # (512x256) and one image after another (600x300)
    for W, H in ((512, 256), (600, 300)):
        rgb, out, stride, bix, _ = _batch(hoh, ctx, W, H, [1, 2, 3], 2)
        assert bix.nbytes() == 0
        assert torch.equal(_decode_batch(hoh, ctx, out, 3, stride, W, H, bix), rgb)
    ctx.close()


def test_stale_batch_index_emptied_by_speed_encode(hoh):
    """an Index that held a -s0 batch, then went through a -s2 batch encode of another shape, is
    empty (no stale image count or stride) and decodes that batch"""
    import torch
    ctx = hoh.Context(0)
    ctx.set_option(hoh.OPT_DECODABLE, 1)
    W, H, n = 512, 256, 3
    _, _, _, ix, _ = _batch(hoh, ctx, W, H, [4, 5], 0)
    assert ix.nbytes() > 0
    stride = hoh.lib().hoh_encode_bound(W, H)
    rgb = torch.cat([hoh.synth_rgb_dev(W, H, sd, 4, ctx=ctx) for sd in (1, 2, 3)])
    out = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hoh.encode_images_async(rgb, n, W, H, out, stride, st, ctx=ctx, index=ix, speed=2)
    torch.cuda.synchronize()
    assert ix.nbytes() == 0 and len(ix.to_bytes()) == 48
    assert torch.equal(_decode_batch(hoh, ctx, out, n, stride, W, H, ix), rgb)
    ctx.close()


def test_truncated_file(hoh, enc):
    _, f, n, _ = enc["A"]
    ctx = hoh.Context(0)
    ix = hoh.Index()
    cut = (n * 6) // 10
    with pytest.raises(hoh.HohError) as ei:
        hoh.build_index(f[:cut].clone(), cut, ctx=ctx, index=ix)
    assert ei.value.code == E_CORRUPT
    assert ix.nbytes() == 0 and len(ix.to_bytes()) == 48
    ctx.close()
