"""Mixed-shape batches with tiled images (hoh_encode_mixed_async / hoh_decode_mixed_async): 64 natural
images with seeded shapes, three quarters tiled (256..1024 pixels a side, at least one side of 512 or
more), one quarter of the small class -- per-image time of ONE mixed call against the two ways
there were before: one synchronous call per image, and one enqueue-only call per image on one
stream with a single wait at the end.  -s0 (decode with and without the side index) and -s1 with
HOH_OPT_DECODABLE.  Host time around loops that end in a device synchronise (what a caller sees),
median of 5; every decode is checked against the images; the stages of one mixed call follow it:
the tile table (mtab), the gather (mgather), the fronts (front, dtable) and the scatter (mscatter).

    python tools/scripts/mixed_tiled_measure.py > profiles/mixed_tiled/measure.txt
"""
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "hoh-ans_amd"))
import torch
import hoh_ans as hoh

REPS = 5
N = 64
ctx = hoh.Context(0)
ctx.set_option(hoh.OPT_SMALL_IMAGES, 1)          # for the single-image calls on small shapes; the mixed calls need none
print("library %s" % hoh.LIBPATH)


def timed(fn, per):
    """ms per image: REPS timed calls of fn (each covers `per` images) after two warm-up calls"""
    fn()
    fn()
    ms = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3 / per)
    return ms


def show(what, ms):
    print("  %-60s min %7.3f  median %7.3f ms/image   (%s)" % (what, min(ms), statistics.median(ms),
                                                               " ".join("%.3f" % v for v in ms)), flush=True)


def stages(fn):
    """device time between the marks of one call; at -s>=1 a mixed call is many jobs: summed by name"""
    ctx.reset_stats()
    ctx.profiling(True)
    fn()
    torch.cuda.synchronize()
    ctx.profiling(False)
    tot = ctx.kernel_stats()
    print("      one call: " + "  ".join("%s %.3f" % (k, v[0]) for k, v in tot.items() if k != "start"), flush=True)


def statuses(st, n, what):
    s = st.cpu().numpy()
    return [hoh.check_status(s[2 * i:2 * i + 2], "%s %d" % (what, i)) for i in range(n)]


rs = random.Random(21)
shapes = []
for i in range(N):
    if i % 4 == 3:
        shapes.append((rs.randint(160, 320), rs.randint(160, 320)))
    else:
        w, h = rs.randint(256, 1024), rs.randint(256, 1024)
        if w < 512 and h < 512:
            w += 512
        shapes.append((w, h))
total, off = hoh.mixed_rgb_bytes(shapes)
rgb = torch.cat([hoh.natural_rgb_dev(w, h, 100 + i, ctx=ctx) for i, (w, h) in enumerate(shapes)])
assert rgb.numel() == total
stride = max(hoh.lib().hoh_encode_bound(w, h) for w, h in shapes)
files = torch.zeros(N * stride, dtype=torch.uint8, device="cuda")
dec = torch.zeros(total, dtype=torch.uint8, device="cuda")
st = torch.zeros(2 * N, dtype=torch.int64, device="cuda")
one = torch.zeros(stride, dtype=torch.uint8, device="cuda")
ntiles = sum((w // 256) * (h // 256) if (w >= 512 or h >= 512) else 1 for w, h in shapes)
print("%d natural images, shapes %s ... (%.2f Mpx, %d tiles, surface %d x %d), %d bytes packed"
      % (N, " ".join("%dx%d" % s for s in shapes[:6]), total / 3e6, ntiles, max(w for w, _ in shapes),
         sum(h for _, h in shapes), total))

for speed in (0, 1):
    ctx.set_option(hoh.OPT_DECODABLE, 1 if speed else 0)
    tag = "-s%d%s" % (speed, " decodable" if speed else "")
    bix = hoh.Index()
    enc_mixed = lambda: hoh.encode_mixed_async(rgb, shapes, files, stride, st, ctx=ctx, index=bix, speed=speed)
    enc_mixed()
    torch.cuda.synchronize()
    sizes = statuses(st, N, "encode")
    print("-- %d mixed shapes %s: %d bytes per file on average (%.2f bits per pixel)"
          % (N, tag, sum(sizes) // N, 8.0 * sum(sizes) / (total / 3)), flush=True)

    def enc_single():
        for i, (w, h) in enumerate(shapes):
            hoh.encode_image(rgb[off[i]:off[i + 1]], w, h, out_dev=one, ctx=ctx, speed=speed)

    def enc_async():
        for i, (w, h) in enumerate(shapes):
            hoh.encode_image_async(rgb[off[i]:off[i + 1]], w, h, files[i * stride:(i + 1) * stride], st[2 * i:2 * i + 2],
                                   ctx=ctx, speed=speed)

    show("encode, one synchronous call per image", timed(enc_single, N))
    show("encode, one enqueue-only call per image, one wait", timed(enc_async, N))
    statuses(st, N, "encode")
    show("encode, one mixed call", timed(enc_mixed, N))
    stages(enc_mixed)
    for index in ((True, False) if speed == 0 else (False,)):
        it = "index" if index else "no index"
        singles = None
        if index:                                              # the files' own indexes, out of the batch's
            singles = [bix.file(i, ctx) for i in range(N)]

        def dec_single():
            for i in range(N):
                hoh.decode_image(files[i * stride:(i + 1) * stride], sizes[i], out_dev=dec[off[i]:off[i + 1]], ctx=ctx,
                                 index=singles[i] if singles else None)

        def dec_async():
            for i, (w, h) in enumerate(shapes):
                hoh.decode_image_async(files[i * stride:(i + 1) * stride], sizes[i], w, h, dec[off[i]:off[i + 1]],
                                       st[2 * i:2 * i + 2], ctx=ctx, index=singles[i] if singles else None)

        dec_mixed = lambda: hoh.decode_mixed_async(files, stride, shapes, dec, st, ctx=ctx, index=bix if index else None)
        dec.zero_()
        show("decode (%s), one synchronous call per image" % it, timed(dec_single, N))
        assert torch.equal(dec, rgb)
        dec.zero_()
        show("decode (%s), one enqueue-only call per image, one wait" % it, timed(dec_async, N))
        statuses(st, N, "decode")
        assert torch.equal(dec, rgb)
        dec.zero_()
        show("decode (%s), one mixed call" % it, timed(dec_mixed, N))
        statuses(st, N, "decode")
        assert torch.equal(dec, rgb)
        stages(dec_mixed)
ctx.close()
