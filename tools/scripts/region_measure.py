"""Region decode on the natural 8192^2 image (-s0 with and without the side index, decodable -s1):
the full decode (the only way to a crop before hoh_decode_region) against region decodes of a
512x512 window at (3000, 3000) (9 tiles), a tile-aligned 256x256 window and the whole image, and
a batch of 8 files with seeded random 512^2 windows.  Device events around loops of calls; every
window is checked against the slice of the image.

    python tools/scripts/region_measure.py [W]
    HOH_LIB=<another build's libhohgpu.so> python tools/scripts/region_measure.py   # full decodes only
"""
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "hoh-ans_amd"))
import torch
import hoh_ans as hoh

W = H = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
HAVE = hasattr(hoh.lib(), "hoh_decode_region")
REPS = 5
print("library %s, region calls %s, image %dx%d natural seed 1" % (hoh.LIBPATH, "present" if HAVE else "absent", W, H))


def timed(fn, iters):
    """ms per call: REPS loops of iters calls between events, after two warm-up calls"""
    fn()
    fn()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return ms


def show(what, ms):
    print("%-58s min %8.3f  median %8.3f ms   (%s)" % (what, min(ms), statistics.median(ms),
                                                       " ".join("%.3f" % v for v in ms)), flush=True)


def stages(ctx, fn):
    ctx.profiling(True)
    fn()
    torch.cuda.synchronize()
    marks = ctx.kernel_ms()          # an enqueue-only call appends to the earlier calls' marks: its own follow the last "start"
    last = max([i for i, (k, _) in enumerate(marks) if k == "start"], default=-1)
    print("      " + "  ".join("%s %.3f" % (k, v) for k, v in marks[last + 1:]), flush=True)
    ctx.profiling(False)


ctx = hoh.Context(0)
rgb = hoh.natural_rgb_dev(W, H, 1, ctx=ctx)
img = rgb.view(H, W, 3)
dec = torch.empty(W * H * 3, dtype=torch.uint8, device="cuda")
WINDOWS = [(3000 * W // 8192, 3000 * H // 8192, 512, 512), (1024 * W // 8192, 2048 * H // 8192, 256, 256), (0, 0, W, H)]

for speed in (0, 1):
    ctx.set_option(hoh.OPT_DECODABLE, 1 if speed else 0)
    ix = hoh.Index() if speed == 0 else None
    out, n, _ = hoh.encode_image(rgb, W, H, ctx=ctx, index=ix, speed=speed)
    torch.cuda.synchronize()
    print("-- -s%d%s: %d bytes" % (speed, " decodable" if speed else "", n), flush=True)
    for index in ([ix, None] if speed == 0 else [None]):
        tag = "-s%d %s" % (speed, "index" if index is not None else "no index")
        iters = 10 if speed == 0 else 3
        show("%s  hoh_decode_image (full)" % tag, timed(lambda: hoh.decode_image(out, n, out_dev=dec, ctx=ctx, index=index), iters))
        assert torch.equal(dec, rgb)
        if not HAVE:
            continue
        for (x, y, w, h) in WINDOWS:
            buf = torch.empty(w * h * 3, dtype=torch.uint8, device="cuda")
            call = lambda: hoh.decode_region(out, n, x, y, w, h, out_dev=buf, ctx=ctx, index=index)
            cover = hoh.region_cover(W, H, x, y, w, h)
            show("%s  hoh_decode_region %dx%d at (%d,%d), %d tiles" % (tag, w, h, x, y, cover[2] * cover[3]),
                 timed(call, iters if w == W else 10 * iters))
            assert torch.equal(buf.view(h, w, 3), img[y:y + h, x:x + w])
            stages(ctx, call)
    del out

# a batch of 8 files, seeded random 512^2 windows, with the index
ctx.set_option(hoh.OPT_DECODABLE, 0)
N = 8
stride = hoh.lib().hoh_encode_bound(W, H)
imgs = torch.empty(N * W * H * 3, dtype=torch.uint8, device="cuda")
for i in range(N):
    imgs[i * W * H * 3:(i + 1) * W * H * 3] = hoh.natural_rgb_dev(W, H, 1 + i, ctx=ctx)
files = torch.empty(N * stride, dtype=torch.uint8, device="cuda")
st = torch.zeros(2 * N, dtype=torch.int64, device="cuda")
bix = hoh.Index()
hoh.encode_images_async(imgs, N, W, H, files, stride, st, ctx=ctx, index=bix)
torch.cuda.synchronize()
print("-- batch of %d -s0 files" % N, flush=True)


def ok():
    s = st.cpu().numpy()
    for i in range(N):
        hoh.check_status(s[2 * i:2 * i + 2], "slot %d" % i)


for index in (bix, None):
    tag = "batch %d %s" % (N, "index" if index is not None else "no index")
    full = torch.empty(N * W * H * 3, dtype=torch.uint8, device="cuda")
    show("%s  hoh_decode_images_async (full)" % tag,
         timed(lambda: hoh.decode_images_async(files, N, stride, W, H, full, st, ctx=ctx, index=index), 3))
    ok()
    assert torch.equal(full, imgs)
    del full
    if not HAVE:
        continue
    rng = random.Random(512)
    w = h = 512
    xy = [(rng.randint(0, W - w), rng.randint(0, H - h)) for _ in range(N)]
    buf = torch.empty(N * w * h * 3, dtype=torch.uint8, device="cuda")
    call = lambda: hoh.decode_regions_async(files, N, stride, W, H, xy, w, h, buf, st, ctx=ctx, index=index)
    nt = sum(c[2] * c[3] for c in (hoh.region_cover(W, H, x, y, w, h) for x, y in xy))
    show("%s  hoh_decode_regions_async 512x512 random, %d tiles" % (tag, nt), timed(call, 30))
    ok()
    for i, (x, y) in enumerate(xy):
        assert torch.equal(buf.view(N, h, w, 3)[i], imgs.view(N, H, W, 3)[i, y:y + h, x:x + w])
    stages(ctx, call)
