"""HOH_OPT_DECODABLE on the natural 8192^2 image: encode time at -s1 / -s4 with the option off and
on (alternated), decode time of the decodable files (events around hoh_decode_image, per-kernel
times from hoh_get_kernel_ms) and the round trip's equality.

    python tools/scripts/decodable_measure.py [W]            # the product library
    HOH_LIB=hoh-ans_amd/lib/libhohgpu_check.so HOH_EXP=128 python tools/scripts/decodable_measure.py W yard
        # the knobs build with k_dgen's one-thread walk (the yardstick): decode part only
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "hoh-ans_amd"))
import torch
import hoh_ans as hoh

W = H = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
yard = len(sys.argv) > 2
REPS = 3
ctx = hoh.Context(0)
rgb = hoh.natural_rgb_dev(W, H, 1, ctx=ctx)
out = torch.empty(hoh.lib().hoh_encode_bound(W, H), dtype=torch.uint8, device="cuda")
dec = torch.empty(W * H * 3, dtype=torch.uint8, device="cuda")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


for speed in (1, 4):
    enc = {0: [], 1: []}
    size = {}
    for rep in range(REPS + 1):
        for on in (0, 1):
            ctx.set_option(hoh.OPT_DECODABLE, on)
            ms, (_, n, _) = timed(lambda: hoh.encode_image(rgb, W, H, out_dev=out, ctx=ctx, speed=speed))
            if rep:
                enc[on].append(ms)
            size[on] = n
    if not yard:
        for on in (0, 1):
            print("encode -s%d decodable=%d: %s ms (min %.2f), %d bytes" %
                  (speed, on, " ".join("%.2f" % v for v in enc[on]), min(enc[on]), size[on]), flush=True)
    n = size[1]                                               # out holds the decodable file
    times = []
    for rep in range(REPS + 1):
        ms, _ = timed(lambda: hoh.decode_image(out, n, out_dev=dec, ctx=ctx))
        if rep:
            times.append(ms)
    print("decode -s%d decodable%s: %s ms (min %.2f), equal %s" %
          (speed, " [one-thread yardstick]" if yard else "", " ".join("%.2f" % v for v in times), min(times),
           bool(torch.equal(dec, rgb))), flush=True)
    ctx.profiling(True)
    hoh.decode_image(out, n, out_dev=dec, ctx=ctx)
    torch.cuda.synchronize()
    print("   " + "  ".join("%s %.3f" % (k, v) for k, v in ctx.kernel_ms()), flush=True)
    ctx.profiling(False)
