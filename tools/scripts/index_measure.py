#!/usr/bin/env python3
"""Measurement: the persistent side index on 8192^2 images at choh -s0 (BASELINE configs[2], the
synthetic image, and configs[4], the natural one).  Writes profiles/index/<label>_<image>.txt.

    python tools/scripts/index_measure.py [label] [legs]     legs: single,pipe (default both)

Per image: file and blob size; hoh_decode_image without an index, with the encoder's recorded
index and with an index built from the file, saved, and loaded again; hoh_index_build itself, with
its stage marks (hoh_set_profiling).  Each timing is the median and the min..max of REP blocks of
N calls, host clock around synchronous calls, after a warm-up of every call shape.  The pipelined
leg is tools/scripts/batch_pipe.py's decode-only schedule (4 contexts x batches of 8, 40 steps):
with the encoder's batch index, with per-file indexes built, saved, loaded and concatenated, and
with none; three runs each, alternating.

A library without hoh_index_build (HOH_LIB=<the parent commit's libhohgpu.so>) runs the legs it
has -- no-index and recorded-index decode, the pipeline with the encoder's index and with none --
which are the parent figures the new ones are set beside."""
import os
import statistics
import sys
import time

LABEL = sys.argv[1] if len(sys.argv) > 1 else "branch"
LEGS = sys.argv[2].split(",") if len(sys.argv) > 2 else ["single", "pipe"]
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "hoh-ans_amd"))
import torch  # noqa: E402
import hoh_ans  # noqa: E402

W = H = 8192
IMG = W * H * 3
REP, N = 3, 10
L = hoh_ans.lib()
HAVE = hasattr(L, "hoh_index_build")
OUT = os.path.join(ROOT, "profiles", "index")
os.makedirs(OUT, exist_ok=True)


def make(kind, seed, ctx):
    return hoh_ans.synth_rgb_dev(W, H, seed, 4, ctx=ctx) if kind == "synthetic" else hoh_ans.natural_rgb_dev(W, H, seed, ctx=ctx)


def timed(fn):
    """median, min, max ms per call over REP blocks of N calls (fn is synchronous)"""
    fn()
    fn()
    v = []
    for _ in range(REP):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(N):
            fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t) / N * 1e3)
    return statistics.median(v), min(v), max(v)


def single(kind, log):
    ctx = hoh_ans.Context(0)
    rgb = make(kind, 1, ctx)
    rec = hoh_ans.Index()
    f, n, _ = hoh_ans.encode_image(rgb, W, H, ctx=ctx, index=rec)
    torch.cuda.synchronize()
    out = torch.empty(IMG, dtype=torch.uint8, device="cuda")
    log("%s 8192^2 -s0: file %d bytes" % (kind, n))
    dctx = hoh_ans.Context(0)                                 # decodes on a context that never encoded

    def dec(ix):
        hoh_ans.decode_image(f, n, out_dev=out, ctx=dctx, index=ix)

    legs = [("decode, no index", None), ("decode, encoder's index", rec)]
    if HAVE:
        E = rec.to_bytes(ctx)
        built = hoh_ans.build_index(f, n, ctx=dctx)
        F = built.to_bytes(dctx)
        log("blob %d bytes (%.2f %% of the file; %d streams, %d checkpoints); built == recorded: %s"
            % (len(F), 100.0 * len(F) / n, int.from_bytes(F[12:16], "little"),
               int.from_bytes(F[32:40], "little"), F == E))
        legs.append(("decode, built + saved + loaded index", hoh_ans.Index.from_bytes(F)))
        t = time.perf_counter()
        hoh_ans.Index.from_bytes(F)
        log("hoh_index_deserialize: %.2f ms; hoh_index_serialize: see below" % ((time.perf_counter() - t) * 1e3))
    res = {}
    for rnd in range(2):                                      # alternate the legs; keep the second round
        for name, ix in legs:
            res[name] = timed(lambda: dec(ix))
    for name, _ in legs:
        log("%-40s %.3f ms  (min %.3f max %.3f over %d x %d)" % ((name,) + res[name] + (REP, N)))
    hoh_ans.decode_image(f, n, out_dev=out, ctx=dctx, index=legs[-1][1])
    torch.cuda.synchronize()
    log("lossless with the last index: %s" % bool(torch.equal(out, rgb)))
    if HAVE:
        ix = hoh_ans.Index()
        for nm, pin in (("adaptive", hoh_ans.NOIX_ADAPTIVE), ("k_ibuild_multi", hoh_ans.NOIX_MULTI),
                        ("k_ibuild_lanes", hoh_ans.NOIX_LANES), ("adaptive", hoh_ans.NOIX_ADAPTIVE)):
            dctx.set_option(hoh_ans.OPT_NOIX_DECODER, pin)
            log("%-40s %.3f ms  (min %.3f max %.3f)"
                % (("hoh_index_build, %s" % nm,) + timed(lambda: hoh_ans.build_index(f, n, ctx=dctx, index=ix))))
        log("%-40s %.3f ms  (min %.3f max %.3f)" % (("hoh_index_serialize",) + timed(lambda: ix.to_bytes(dctx))))
        dctx.profiling(True)
        dctx.reset_stats()
        for _ in range(N):
            hoh_ans.build_index(f, n, ctx=dctx, index=ix)
        st = dctx.kernel_stats()
        dctx.profiling(False)
        log("hoh_index_build stages (ms per call): " +
            ", ".join("%s %.3f" % (k, v[0] / max(v[1], 1)) for k, v in st.items()))
    ctx.close()
    dctx.close()


def pipe(log, D=4, B=8, K=40):
    stride = L.hoh_encode_bound(W, H)
    slots = []
    for k in range(D):
        c = hoh_ans.Context(0)
        s = torch.cuda.Stream()
        rgb = torch.empty(B * IMG, dtype=torch.uint8, device="cuda")
        for b in range(B):
            rgb[b * IMG:(b + 1) * IMG] = hoh_ans.synth_rgb_dev(W, H, 1 + k * B + b, 4, ctx=c)
        out = torch.empty(B * stride, dtype=torch.uint8, device="cuda")
        dec = torch.empty(B * IMG, dtype=torch.uint8, device="cuda")
        st = torch.zeros(4 * B, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rec = hoh_ans.Index()
        hoh_ans.encode_images_async(rgb, B, W, H, out, stride, st[:2 * B], ctx=c, index=rec)
        torch.cuda.synchronize()
        sizes = [int(v) for v in st[1:2 * B:2].cpu()]
        cat = None
        if HAVE:
            blobs = []
            for b in range(B):                                # what a loader holds: N files and N sidecars
                blobs.append(hoh_ans.build_index(out[b * stride:(b + 1) * stride], sizes[b], ctx=c).to_bytes(c))
            cat = hoh_ans.Index.concat([hoh_ans.Index.from_bytes(x) for x in blobs], stride)
            assert cat.to_bytes() == rec.to_bytes(c), "concatenated index differs from the batch encoder's"
        slots.append((c, s, rgb, out, dec, st, {"encoder's index": rec, "concatenated loaded indexes": cat, "no index": None}))
    names = ["encoder's index", "no index"] + (["concatenated loaded indexes"] if HAVE else [])

    def run(name, n):
        for i in range(n):
            c, s, rgb, out, dec, st, ixs = slots[i % D]
            with torch.cuda.stream(s):
                hoh_ans.decode_images_async(out, B, stride, W, H, dec, st[2 * B:], ctx=c, index=ixs[name])

    res = {k: [] for k in names}
    for rnd in range(3):
        for name in names:
            run(name, D)
            torch.cuda.synchronize()
            t = time.perf_counter()
            run(name, K)
            torch.cuda.synchronize()
            el = time.perf_counter() - t
            res[name].append(IMG * B * K / el / 1e9)
            ok = all(bool(torch.equal(x[4], x[2])) for x in slots)
            assert ok, name
    for name in names:
        v = res[name]
        log("decode-only pipeline, %d contexts x %d images, %d steps, %-28s %s GB/s raw (median %.1f), lossless"
            % (D, B, K, name + ":", " ".join("%.1f" % x for x in v), statistics.median(v)))


def main():
    for kind in ("synthetic", "natural"):
        if "single" not in LEGS:
            break
        with open(os.path.join(OUT, "%s_%s.txt" % (LABEL, kind)), "w") as fo:
            def log(s):
                print(s, flush=True)
                fo.write(s + "\n")
                fo.flush()
            log("# %s, library %s" % (L.hoh_version().decode(), LABEL))
            single(kind, log)
    if "pipe" in LEGS:
        with open(os.path.join(OUT, "%s_pipeline.txt" % LABEL), "w") as fo:
            def log(s):
                print(s, flush=True)
                fo.write(s + "\n")
                fo.flush()
            log("# %s, library %s" % (L.hoh_version().decode(), LABEL))
            pipe(log)


if __name__ == "__main__":
    main()
