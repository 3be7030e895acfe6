"""Small images (HOH_OPT_SMALL_IMAGES): 64 natural 224^2 images, then 16 of 511^2 -- per-image time of
encode and decode one image at a time through the synchronous calls against one batched call, decode
with and without the side index, at -s0 and at -s1 with HOH_OPT_DECODABLE.  Host time around loops
that end in a device synchronise (what a caller sees: the synchronous calls pay a host round trip
each, which is the point of the batch); every decode is checked against the images; the stages of
one batched call follow each group.

    python tools/scripts/small_images_measure.py > profiles/small_images/measure.txt
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "hoh-ans_amd"))
import torch
import hoh_ans as hoh

REPS = 5
ctx = hoh.Context(0)
ctx.set_option(hoh.OPT_SMALL_IMAGES, 1)
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
    print("  %-52s min %7.3f  median %7.3f ms/image   (%s)" % (what, min(ms), statistics.median(ms),
                                                               " ".join("%.3f" % v for v in ms)), flush=True)


def stages(fn):
    ctx.reset_stats()                # folds the marks earlier enqueue-only calls appended
    ctx.profiling(True)
    fn()
    torch.cuda.synchronize()
    marks = ctx.kernel_ms()
    last = max([i for i, (k, _) in enumerate(marks) if k == "start"], default=-1)
    print("      one call: " + "  ".join("%s %.3f" % (k, v) for k, v in marks[last + 1:]), flush=True)
    ctx.profiling(False)


def statuses(st, n, what):
    s = st.cpu().numpy()
    return [hoh.check_status(s[2 * i:2 * i + 2], "%s %d" % (what, i)) for i in range(n)]


for (W, H, n) in ((224, 224, 64), (511, 511, 16)):
    img = W * H * 3
    rgb = hoh.natural_rgb_dev(W, H * n, 1, ctx=ctx)            # n images: the rows of one tall natural image
    stride = hoh.lib().hoh_encode_bound(W, H)
    files = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    dec = torch.zeros(n * img, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    one = torch.zeros(stride, dtype=torch.uint8, device="cuda")
    for speed in (0, 1):
        ctx.set_option(hoh.OPT_DECODABLE, 1 if speed else 0)
        tag = "-s%d%s" % (speed, " decodable" if speed else "")
        bix = hoh.Index()
        enc_batch = lambda: hoh.encode_images_async(rgb, n, W, H, files, stride, st, ctx=ctx, index=bix, speed=speed)
        enc_batch()
        torch.cuda.synchronize()
        sizes = statuses(st, n, "encode")
        print("-- %d x %dx%d %s: %d bytes per file on average (%.2f bits per pixel)"
              % (n, W, H, tag, sum(sizes) // n, 8.0 * sum(sizes) / (n * W * H)), flush=True)

        def enc_single():
            for i in range(n):
                hoh.encode_image(rgb[i * img:(i + 1) * img], W, H, out_dev=one, ctx=ctx, speed=speed)

        show("encode, one synchronous call per image", timed(enc_single, n))
        show("encode, one batched call", timed(enc_batch, n))
        stages(enc_batch)
        for index in ((bix, None) if speed == 0 else (None,)):
            it = "index" if index is not None else "no index"
            singles = None
            if index is not None:                              # the single files' own indexes
                singles = []
                for i in range(n):
                    ix = hoh.Index()
                    hoh.encode_image(rgb[i * img:(i + 1) * img], W, H, out_dev=one, ctx=ctx, index=ix)
                    singles.append(ix)

            def dec_single():
                for i in range(n):
                    hoh.decode_image(files[i * stride:(i + 1) * stride], sizes[i], out_dev=dec[i * img:(i + 1) * img], ctx=ctx,
                                     index=singles[i] if singles else None)

            dec_batch = lambda: hoh.decode_images_async(files, n, stride, W, H, dec, st, ctx=ctx, index=index)
            dec.zero_()
            show("decode (%s), one synchronous call per image" % it, timed(dec_single, n))
            assert torch.equal(dec, rgb)
            dec.zero_()
            show("decode (%s), one batched call" % it, timed(dec_batch, n))
            statuses(st, n, "decode")
            assert torch.equal(dec, rgb)
            stages(dec_batch)
ctx.close()
