"""Mixed-shape batches (hoh_encode_mixed_async / hoh_decode_mixed_async): 64 natural images with
seeded shapes of 160..320 pixels on each side -- per-image time of one mixed call against one
synchronous call per image (the only other way for n shapes) and against the uniform batch of
64 x 224^2 as the per-image reference, decode with and without the side index, at -s0 and at -s1
with HOH_OPT_DECODABLE.  Host time around loops that end in a device synchronise (what a caller
sees); every decode is checked against the images; the stages of one call follow each group, the
gather (mgather) and the scatter (mscatter) on their own: what the staging surface costs.

    python tools/scripts/mixed_batch_measure.py > profiles/mixed_batch/measure.txt
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
ctx.set_option(hoh.OPT_SMALL_IMAGES, 1)          # for the single-image and uniform calls; the mixed calls need none
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
    print("  %-56s min %7.3f  median %7.3f ms/image   (%s)" % (what, min(ms), statistics.median(ms),
                                                               " ".join("%.3f" % v for v in ms)), flush=True)


def stages(fn):
    """device time between the marks of one call; at -s>=1 a mixed call is many jobs: summed by name"""
    ctx.reset_stats()                # folds the marks earlier enqueue-only calls appended
    ctx.profiling(True)
    fn()
    torch.cuda.synchronize()
    ctx.profiling(False)
    tot = ctx.kernel_stats()
    print("      one call: " + "  ".join("%s %.3f" % (k, v[0]) for k, v in tot.items() if k != "start"), flush=True)


def statuses(st, n, what):
    s = st.cpu().numpy()
    return [hoh.check_status(s[2 * i:2 * i + 2], "%s %d" % (what, i)) for i in range(n)]


rs = random.Random(20)
shapes = [(rs.randint(160, 320), rs.randint(160, 320)) for _ in range(N)]
total, off = hoh.mixed_rgb_bytes(shapes)
rgb = torch.cat([hoh.natural_rgb_dev(w, h, 100 + i, ctx=ctx) for i, (w, h) in enumerate(shapes)])
assert rgb.numel() == total
stride = max(hoh.lib().hoh_encode_bound(w, h) for w, h in shapes)
files = torch.zeros(N * stride, dtype=torch.uint8, device="cuda")
dec = torch.zeros(total, dtype=torch.uint8, device="cuda")
st = torch.zeros(2 * N, dtype=torch.int64, device="cuda")
one = torch.zeros(stride, dtype=torch.uint8, device="cuda")
print("%d natural images, shapes %s ... (%.1f pixels a side on average), %d bytes packed"
      % (N, " ".join("%dx%d" % s for s in shapes[:6]), (sum(w * h for w, h in shapes) / N) ** 0.5, total))

# the per-image reference: the uniform batch of 64 x 224^2
UW = UH = 224
urgb = hoh.natural_rgb_dev(UW, UH * N, 1, ctx=ctx)
ustride = hoh.lib().hoh_encode_bound(UW, UH)
ufiles = torch.zeros(N * ustride, dtype=torch.uint8, device="cuda")
udec = torch.zeros(N * UW * UH * 3, dtype=torch.uint8, device="cuda")

for speed in (0, 1):
    ctx.set_option(hoh.OPT_DECODABLE, 1 if speed else 0)
    tag = "-s%d%s" % (speed, " decodable" if speed else "")
    bix, uix = hoh.Index(), hoh.Index()
    enc_mixed = lambda: hoh.encode_mixed_async(rgb, shapes, files, stride, st, ctx=ctx, index=bix, speed=speed)
    enc_mixed()
    torch.cuda.synchronize()
    sizes = statuses(st, N, "encode")
    print("-- %d mixed shapes %s: %d bytes per file on average (%.2f bits per pixel)"
          % (N, tag, sum(sizes) // N, 8.0 * sum(sizes) / (total / 3)), flush=True)

    def enc_single():
        for i, (w, h) in enumerate(shapes):
            hoh.encode_image(rgb[off[i]:off[i + 1]], w, h, out_dev=one, ctx=ctx, speed=speed)

    enc_uniform = lambda: hoh.encode_images_async(urgb, N, UW, UH, ufiles, ustride, st, ctx=ctx, index=uix, speed=speed)
    show("encode, one synchronous call per image", timed(enc_single, N))
    show("encode, one mixed call", timed(enc_mixed, N))
    stages(enc_mixed)
    show("encode, uniform batch of 64 x 224^2", timed(enc_uniform, N))
    stages(enc_uniform)
    for index in ((True, False) if speed == 0 else (False,)):
        it = "index" if index else "no index"
        singles = None
        if index:                                              # the single files' own indexes
            singles = []
            for i, (w, h) in enumerate(shapes):
                ix = hoh.Index()
                hoh.encode_image(rgb[off[i]:off[i + 1]], w, h, out_dev=one, ctx=ctx, index=ix)
                singles.append(ix)

        def dec_single():
            for i in range(N):
                hoh.decode_image(files[i * stride:(i + 1) * stride], sizes[i], out_dev=dec[off[i]:off[i + 1]], ctx=ctx,
                                 index=singles[i] if singles else None)

        dec_mixed = lambda: hoh.decode_mixed_async(files, stride, shapes, dec, st, ctx=ctx, index=bix if index else None)
        dec_uniform = lambda: hoh.decode_images_async(ufiles, N, ustride, UW, UH, udec, st, ctx=ctx,
                                                      index=uix if index else None)
        dec.zero_()
        show("decode (%s), one synchronous call per image" % it, timed(dec_single, N))
        assert torch.equal(dec, rgb)
        dec.zero_()
        show("decode (%s), one mixed call" % it, timed(dec_mixed, N))
        statuses(st, N, "decode")
        assert torch.equal(dec, rgb)
        stages(dec_mixed)
        udec.zero_()
        show("decode (%s), uniform batch of 64 x 224^2" % it, timed(dec_uniform, N))
        statuses(st, N, "decode")
        assert torch.equal(udec, urgb)
        stages(dec_uniform)
ctx.close()
