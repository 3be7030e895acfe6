"""GPU: region decode (hoh_decode_region / _async / hoh_decode_regions_async and `dhoh --region`).
The codec is lossless, so the expected pixels of every window are the numpy slice of the image
that was encoded -- never the output of another call of the library."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DHOH = os.path.join(ROOT, "hoh-ans_amd", "bin", "dhoh")
E_ARG, E_CAP, E_UNSUPPORTED, E_CORRUPT = 1, 2, 6, 7
FILL = 0xA5


@pytest.fixture(scope="module")
def hoh():
    import torch  # noqa: F401  (before the first context: torch brings its own HIP runtime)
    import hoh_ans
    return hoh_ans


@pytest.fixture(scope="module")
def ctxs(hoh):
    """one context per way of decoding: with the encoder's index (the encoding context), with an
    index loaded from its blob (a fresh context), and without an index under each pinned decoder"""
    c = {k: hoh.Context(0) for k in ("enc", "loaded", "lanes", "multi", "wave")}
    c["lanes"].set_option(hoh.OPT_NOIX_DECODER, hoh.NOIX_LANES)
    c["multi"].set_option(hoh.OPT_NOIX_DECODER, hoh.NOIX_MULTI)
    c["wave"].set_option(hoh.OPT_NOIX_DECODER, hoh.NOIX_WAVE)
    yield c
    for v in c.values():
        v.close()


class File:
    def __init__(self, hoh, ctx, img, speed=0, index=True):
        import torch
        self.img = img
        self.H, self.W = img.shape[:2]
        d = torch.from_numpy(img.reshape(-1).copy()).cuda()
        self.index = hoh.Index() if index else None
        self.dev, self.size, _ = hoh.encode_image(d, self.W, self.H, ctx=ctx, index=self.index, speed=speed)
        torch.cuda.synchronize()
        self.blob = self.index.to_bytes(ctx) if index else None
        self.loaded = hoh.Index.from_bytes(self.blob) if index else None
        _, self.xt, self.yt, self.tw, self.th = hoh.tiling(self.W, self.H)

    def bytes(self):
        return self.dev[:self.size].cpu().numpy().tobytes()

    def windows(self):
        W, H, tw, th = self.W, self.H, self.tw, self.th
        return [(0, 0, W, H),                       # the whole image
                (tw + 5, th + 7, 1, 1),             # one pixel inside a tile
                (10, 20, 100, 50),                  # inside one tile
                (tw - 6, th - 6, 12, 12),           # the four-tile corner at the first seam
                (0, th + 3, W, 1),                  # a full-width single row
                (W - 1, 0, 1, H),                   # the last column
                (0, H - 1, W, 1),                   # the last row
                (tw - 1, 7, 3, 295)]                # odd x and w across a vertical seam


def _varint(data, p):
    b0 = data[p]
    if not b0 & 0x80:
        return b0, p + 1
    b1 = data[p + 1]
    if not b1 & 0x80:
        return ((b0 & 0x7f) << 7) + b1, p + 2
    return ((b0 & 0x7f) << 14) + ((b1 & 0x7f) << 7) + data[p + 2], p + 3


def _tile_offsets(data):
    """byte offset of every tile of a .hoh, from its varint size table (choh.cpp:437-498)"""
    p = 6
    _, p = _varint(data, p)
    _, p = _varint(data, p)
    nt = (data[p] + 1) * (data[p + 1] + 1)
    p += 2
    sizes = []
    for _ in range(nt - 1):
        v, p = _varint(data, p)
        sizes.append(v)
    return [p + sum(sizes[:i]) for i in range(nt)]


@pytest.fixture(scope="module")
def files(hoh, ctxs):
    from hoh_ans.natural import natural_rgb
    from hoh_ans.synth import synth_rgb
    dctx = hoh.Context(0)
    dctx.set_option(hoh.OPT_DECODABLE, 1)
    f = {"A": File(hoh, ctxs["enc"], synth_rgb(768, 512, seed=31, noise=4)),
         "B": File(hoh, ctxs["enc"], synth_rgb(1000, 600, seed=32, noise=4)),
         "C": File(hoh, ctxs["enc"], natural_rgb(768, 512, seed=33)),
         "D": File(hoh, dctx, natural_rgb(768, 512, seed=34), speed=2, index=False)}
    assert f["B"].windows()[-1] == (333, 7, 3, 295) and (f["B"].tw, f["B"].th) == (334, 300)
    yield f
    dctx.close()


def _check_window(hoh, f, win, ctx, index, odd_pitch):
    """decode one window; the bytes of its rows equal the slice, every other byte keeps the fill"""
    import torch
    x, y, w, h = win
    pitch = w * 3 + (5 if odd_pitch else 0)
    need = (h - 1) * pitch + w * 3
    buf = torch.full((need + 7,), FILL, dtype=torch.uint8, device="cuda")
    out, W, H = hoh.decode_region(f.dev, f.size, x, y, w, h, out_dev=buf[:need], pitch=pitch, ctx=ctx, index=index)
    torch.cuda.synchronize()
    assert (W, H) == (f.W, f.H)
    got = buf.cpu().numpy()
    want = np.full(need + 7, FILL, np.uint8)
    rows = f.img[y:y + h, x:x + w].reshape(h, w * 3)
    for r in range(h):
        want[r * pitch:r * pitch + w * 3] = rows[r]
    assert np.array_equal(got, want), (win, pitch)
    if pitch % 3 == 0:
        assert tuple(out.shape) == (h, w, 3) and np.array_equal(out.cpu().numpy(), f.img[y:y + h, x:x + w])
    else:
        assert out.dim() == 1


MODES = ["enc", "loaded", "lanes", "multi", "wave"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_windows(hoh, ctxs, files, name, mode):
    f, ctx = files[name], ctxs[mode]
    index = {"enc": f.index, "loaded": f.loaded}.get(mode)
    ctx.profiling(True)
    try:
        for win in f.windows():
            for odd in (False, True):
                _check_window(hoh, f, win, ctx, index, odd)
                stages = [k for k, _ in ctx.kernel_ms()]
                assert "drans" in stages and "dcrop" in stages, stages
    finally:
        ctx.profiling(False)


def test_windows_general_tiles(hoh, ctxs, files):
    f = files["D"]
    for win in f.windows():
        for odd in (False, True):
            _check_window(hoh, f, win, ctxs["lanes"], None, odd)


@pytest.mark.parametrize("with_index", [False, True])
def test_untouched_tiles_are_not_read(hoh, ctxs, files, with_index):
    import torch
    f = files["A"]
    data = bytearray(f.bytes())
    data[_tile_offsets(data)[5]] = 1                      # tile 5 now announces nested tiling
    dev = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()
    ctx = ctxs["enc"]
    ix = f.index if with_index else None
    with pytest.raises(hoh.HohError) as e:
        hoh.decode_image(dev, len(data), ctx=ctx, index=ix)
    assert e.value.code == E_UNSUPPORTED
    x, y, w, h = 200, 10, 100, 100                        # tiles 0 and 1
    assert hoh.region_cover(f.W, f.H, x, y, w, h) == (0, 0, 2, 1)
    out, _, _ = hoh.decode_region(dev, len(data), x, y, w, h, ctx=ctx, index=ix)
    assert np.array_equal(out.cpu().numpy(), f.img[y:y + h, x:x + w])
    with pytest.raises(hoh.HohError) as e:
        hoh.decode_region(dev, len(data), 600, 300, 10, 10, ctx=ctx, index=ix)   # inside tile 5
    assert e.value.code == E_UNSUPPORTED


def test_covered_streams_use_their_checkpoints(hoh, ctxs, files):
    """A checkpoint of tile 4's G plane altered in the index blob: a window inside tile 4 fails
    (its stream starts from the index's states, found under the tile's number in the whole file's
    index), a window inside tile 0 does not."""
    f = files["A"]
    blob = bytearray(f.blob)
    nstreams = struct.unpack_from("<I", blob, 12)[0]
    assert nstreams == 7 * f.xt * f.yt
    s, first = 4 * 7 + 3, 0
    for i in range(s):
        _, n, mode = struct.unpack_from("<QII", blob, 48 + 24 * i)
        first += (n + 255) // 256 if mode == 1 else 0
    _, n, mode = struct.unpack_from("<QII", blob, 48 + 24 * s)
    assert mode == 1 and n > 512
    at = 48 + 24 * nstreams + 12 * (first + 1)
    blob[at] ^= 1
    bad = hoh.Index.from_bytes(bytes(blob))
    ctx = ctxs["loaded"]
    out, _, _ = hoh.decode_region(f.dev, f.size, 10, 20, 100, 50, ctx=ctx, index=bad)
    assert np.array_equal(out.cpu().numpy(), f.img[20:70, 10:110])
    with pytest.raises(hoh.HohError) as e:
        hoh.decode_region(f.dev, f.size, 300, 300, 20, 20, ctx=ctx, index=bad)
    assert e.value.code == E_CORRUPT
    out, _, _ = hoh.decode_region(f.dev, f.size, 300, 300, 20, 20, ctx=ctx, index=f.loaded)
    assert np.array_equal(out.cpu().numpy(), f.img[300:320, 300:320])


@pytest.mark.parametrize("name", ["A", "B"])
def test_async(hoh, ctxs, files, name):
    import torch
    f, ctx = files[name], ctxs["enc"]
    wins = f.windows()
    st = torch.zeros(2 * len(wins) * 2, dtype=torch.int64, device="cuda")
    outs = []
    for k, (x, y, w, h) in enumerate(wins):
        for q, ix in enumerate((f.index, None)):
            buf = torch.full((h * w * 3,), FILL, dtype=torch.uint8, device="cuda")
            slot = st[2 * (2 * k + q):2 * (2 * k + q) + 2]
            outs.append((hoh.decode_region_async(f.dev, f.size, f.W, f.H, x, y, w, h, buf, slot, ctx=ctx, index=ix),
                         (x, y, w, h)))
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    for i, (out, (x, y, w, h)) in enumerate(outs):
        assert hoh.check_status(s[2 * i:2 * i + 2], "region %d" % i) == w * h * 3
        assert np.array_equal(out.cpu().numpy(), f.img[y:y + h, x:x + w]), (x, y, w, h)


def test_async_wrong_width_is_corrupt(hoh, ctxs, files):
    import torch
    f = files["A"]
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    buf = torch.full((10 * 10 * 3,), FILL, dtype=torch.uint8, device="cuda")
    hoh.decode_region_async(f.dev, f.size, f.W + 256, f.H, 0, 0, 10, 10, buf, st, ctx=ctxs["enc"])
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == [E_CORRUPT, 0]
    assert bool((buf == FILL).all())


def _status_ok(hoh, st, n, nbytes):
    s = st.cpu().numpy()
    for i in range(n):
        assert hoh.check_status(s[2 * i:2 * i + 2], "slot %d" % i) == nbytes


def test_batch_stacked_files(hoh, ctxs):
    import torch
    from hoh_ans.synth import synth_rgb
    W, H, n, w, h = 512, 256, 3, 200, 100
    xy = [(0, 0), (156, 100), (312, 156)]
    assert [hoh.region_cover(W, H, x, y, w, h)[2:] for x, y in xy] == [(1, 1), (2, 1), (1, 1)]
    imgs = np.stack([synth_rgb(W, H, seed=40 + i, noise=4) for i in range(n)])
    rgb = torch.from_numpy(imgs.reshape(-1).copy()).cuda()
    stride = hoh.lib().hoh_encode_bound(W, H)
    files_dev = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    ctx = ctxs["enc"]
    ix = hoh.Index()
    hoh.encode_images_async(rgb, n, W, H, files_dev, stride, st, ctx=ctx, index=ix)
    torch.cuda.synchronize()
    assert ix.nbytes() > 0
    for index in (ix, None):
        for pitch in (w * 3, w * 3 + 5):
            need = (n * h - 1) * pitch + w * 3
            buf = torch.full((need + 7,), FILL, dtype=torch.uint8, device="cuda")
            st.zero_()
            hoh.decode_regions_async(files_dev, n, stride, W, H, xy, w, h, buf[:need], st, pitch=pitch, ctx=ctx,
                                     index=index)
            torch.cuda.synchronize()
            _status_ok(hoh, st, n, w * h * 3)
            want = np.full(need + 7, FILL, np.uint8)
            for i, (x, y) in enumerate(xy):
                rows = imgs[i, y:y + h, x:x + w].reshape(h, w * 3)
                for r in range(h):
                    o = (i * h + r) * pitch
                    want[o:o + w * 3] = rows[r]
            assert np.array_equal(buf.cpu().numpy(), want), (index is not None, pitch)
    # the index of a batch of another n does not serve this one
    ix2 = hoh.Index()
    out2 = torch.zeros(2 * stride, dtype=torch.uint8, device="cuda")
    hoh.encode_images_async(rgb, 2, W, H, out2, stride, st[:4], ctx=ctx, index=ix2)
    torch.cuda.synchronize()
    buf = torch.full((n * h * w * 3,), FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(hoh.HohError) as e:
        hoh.decode_regions_async(files_dev, n, stride, W, H, xy, w, h, buf, st, ctx=ctx, index=ix2)
    assert e.value.code == E_ARG
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())


def test_batch_files_that_do_not_stack(hoh, ctxs):
    import torch
    from hoh_ans.synth import synth_rgb
    W, H, n, w, h = 600, 300, 3, 200, 100
    xy = [(0, 0), (250, 150), (400, 200)]
    imgs = [synth_rgb(W, H, seed=50 + i, noise=4) for i in range(n)]
    stride = hoh.lib().hoh_encode_bound(W, H)
    files_dev = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    ctx = ctxs["lanes"]
    for i in range(n):
        d = torch.from_numpy(imgs[i].reshape(-1).copy()).cuda()
        hoh.encode_image(d, W, H, out_dev=files_dev[i * stride:(i + 1) * stride], ctx=ctx)
    st = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    out = hoh.decode_regions_async(files_dev, n, stride, W, H, xy, w, h, None, st, ctx=ctx)
    torch.cuda.synchronize()
    _status_ok(hoh, st, n, w * h * 3)
    got = out.cpu().numpy()
    for i, (x, y) in enumerate(xy):
        assert np.array_equal(got[i], imgs[i][y:y + h, x:x + w]), i


def test_batch_of_one_equals_the_single_call(hoh, ctxs, files):
    import torch
    f, ctx = files["C"], ctxs["enc"]
    x, y, w, h = 250, 250, 300, 200
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    for index in (f.index, None):
        one = hoh.decode_regions_async(f.dev, 1, f.size, f.W, f.H, [(x, y)], w, h, None, st, ctx=ctx, index=index)
        single, _, _ = hoh.decode_region(f.dev, f.size, x, y, w, h, ctx=ctx, index=index)
        torch.cuda.synchronize()
        _status_ok(hoh, st, 1, w * h * 3)
        assert np.array_equal(one.cpu().numpy()[0], f.img[y:y + h, x:x + w])
        assert np.array_equal(single.cpu().numpy(), f.img[y:y + h, x:x + w])


def test_arguments(hoh, ctxs, files):
    import torch
    f, ctx = files["A"], ctxs["enc"]
    W, H = f.W, f.H
    buf = torch.full((64 * 64 * 3 + 64,), FILL, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * 257,), -1, dtype=torch.int64, device="cuda")

    def codes(x, y, w, h, pitch=None, cap=None):
        """the code of each call for one window (the batch call takes no cap: left out when one is given)"""
        out = buf if cap is None else buf[:cap]
        calls = [lambda: hoh.decode_region(f.dev, f.size, x, y, w, h, out_dev=out, pitch=pitch, ctx=ctx),
                 lambda: hoh.decode_region_async(f.dev, f.size, W, H, x, y, w, h, out, st[:2], pitch=pitch, ctx=ctx)]
        if cap is None:
            calls.append(lambda: hoh.decode_regions_async(f.dev, 1, f.size, W, H, [(x, y)], w, h, buf, st[:2],
                                                          pitch=pitch, ctx=ctx))
        got = []
        for call in calls:
            with pytest.raises(hoh.HohError) as e:
                call()
            got.append(e.value.code)
        return got

    for win in [(0, 0, 0, 8), (0, 0, 8, 0), (0, 0, -8, 8), (0, 0, 8, -8),      # empty / negative sizes
                (W - 8 + 1, 0, 8, 8), (0, H - 8 + 1, 8, 8),                   # one pixel past an edge
                (-1, 0, 8, 8), (0, -1, 8, 8)]:
        assert codes(*win) == [E_ARG] * 3, win
    assert codes(0, 0, 8, 8, pitch=8 * 3 - 1) == [E_ARG] * 3                  # a pitch one byte short
    need = 7 * (8 * 3 + 5) + 8 * 3
    assert codes(0, 0, 8, 8, pitch=8 * 3 + 5, cap=need - 1) == [E_CAP] * 2    # a cap one byte short
    out, _, _ = hoh.decode_region(f.dev, f.size, 0, 0, 8, 8, out_dev=torch.zeros(need, dtype=torch.uint8, device="cuda"),
                                  pitch=8 * 3 + 5, ctx=ctx)                   # exactly enough
    assert out.dim() == 1
    for n in (0, -1, 257):
        xy = [(0, 0)] * max(n, 0)
        with pytest.raises(hoh.HohError) as e:
            hoh.decode_regions_async(torch.zeros(max(n, 1) * 16, dtype=torch.uint8, device="cuda"), n, 16, W, H, xy, 1, 1,
                                     torch.full((max(n, 1) * 3,), FILL, dtype=torch.uint8, device="cuda"), st, ctx=ctx)
        assert e.value.code == E_ARG, n
    # an untiled shape
    with pytest.raises(hoh.HohError) as e:
        hoh.decode_region_async(f.dev, f.size, 300, 300, 0, 0, 8, 8, buf, st[:2], ctx=ctx)
    assert e.value.code == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((buf == FILL).all()) and bool((st == -1).all())


def test_repeat_call_allocates_nothing(hoh, ctxs, files):
    import torch
    f, ctx = files["C"], ctxs["multi"]
    out = torch.zeros(300 * 200 * 3, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    hoh.decode_region(f.dev, f.size, 250, 250, 300, 200, out_dev=out, ctx=ctx)
    hoh.decode_regions_async(f.dev, 1, f.size, f.W, f.H, [(250, 250)], 300, 200, out, st, ctx=ctx)
    torch.cuda.synchronize()
    before = hoh.device_alloc_count()
    hoh.decode_region(f.dev, f.size, 250, 250, 300, 200, out_dev=out, ctx=ctx)
    hoh.decode_regions_async(f.dev, 1, f.size, f.W, f.H, [(250, 250)], 300, 200, out, st, ctx=ctx)
    torch.cuda.synchronize()
    assert hoh.device_alloc_count() == before


def test_cli_region(hoh, ctxs, files, tmp_path):
    f = files["A"]
    hohf, hix = tmp_path / "a.hoh", tmp_path / "a.hix"
    hohf.write_bytes(f.bytes())
    hix.write_bytes(f.blob)
    x, y, w, h = 100, 50, 300, 200
    want = f.img[y:y + h, x:x + w].tobytes()

    def run(*extra):
        return subprocess.run([DHOH, str(hohf), str(tmp_path / "o.rgb")] + [str(a) for a in extra], capture_output=True,
                              text=True, timeout=120)

    for extra in ((), ("--index", hix)):
        r = run("--region", "%d,%d,%d,%d" % (x, y, w, h), *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        assert (tmp_path / "o.rgb").read_bytes() == want
    for bad in ("100,50,300", "a,b,c,d", "100,50,300,200,1", "0,0,0,10", "700,0,100,10", "-1,0,5,5"):
        r = run("--region", bad)
        assert r.returncode == 1 and "usage" in r.stdout, (bad, r.stdout)
