"""The decoder's rANS chain kernels (k_drans, k_drans_wave, k_drans_multi, k_drans_lanes,
k_ibuild_lanes / k_ibuild_multi) against streams no image produces: tests/designed_streams.py builds
-s0-shaped tiles whose residual streams have chosen frequency tables at prob_bits 8..15.

Designs: (a) single symbol, (b) two symbols with frequencies 2^pb - 1 and 1, (c) / (d) a burst of
frequency-1 symbols below / above one peak symbol (16-symbol groups that read 8 payload words, the
payload rings' bound, next to thousands that read none; 64 symbol starts in one 64-slot bucket at
either end of the range), (e) equal frequencies (every start on a bucket edge), (f) all 512
symbols of a 9-bit plane present, (g) a geometric body on a narrow support at the prob_bits the
others leave out.  Layouts: 256-wide tiles (blocked planes), 300 x 300 tiles (flat, a last segment
of 912 symbols), LZ tiles with compacted planes of 761 and 9467 symbols.

test_cases_have_what_they_claim and test_helper_reads_its_own_files need no GPU.  Every comparison
is exact; nothing here measures time."""
import numpy as np
import pytest

import decodable_ref as dr
import designed_streams as ds

gpu = pytest.mark.gpu
NOIX = ["lanes", "multi", "wave", "adaptive"]
BATCH = ["F0", "F1", "F2"]                                    # the files of one shape


# ---------------------------------------------------------------- CPU: the inputs are what they say

def test_cases_have_what_they_claim(orc):
    cs, fs = ds.cases(), ds.files()
    covered = {8: set(), 9: set()}
    walks, pay_mod4 = {}, set()
    for data, _, offs in fs.values():
        for name, toff in offs:
            c = cs[name]
            h, w, _ = c["px"].shape
            t = dr.parse_tile(c["tile"], 0, len(c["tile"]), w, h)
            assert t["mode"] == 128 and t["nlz"] == 3
            assert all(L["masks"] == [0x0010] and not L["mapped"] for L in t["layers"])
            if c["design"] == "lz":                           # every compacted plane is a rANS stream
                assert t["matches"] and [L["pb"] for L in t["layers"]] == list(c["pbs"])
                continue
            k = c["plane"]
            L = t["layers"][k]
            rng = 1 << c["depth"]
            assert L["pb"] == c["pb"], (name, L["pb"])        # rANS (None: stored) at the intended prob_bits
            assert np.array_equal(L["res"], c["res"]) and (k == 0) == (c["depth"] == 8)
            assert L["stream"] == orc.encode_entropy(c["res"], rng, c["pb"])
            covered[c["depth"]].add(c["pb"])
            wk = walks[name] = ds.rans_walk(c["res"], rng, c["pb"])
            pay = wk["words"].tobytes()
            assert L["stream"][-len(pay):] == pay, name       # the model is the oracle's coder
            end = toff + ds.stream_ends(t, len(c["tile"]))[k]
            assert data[end - len(pay):end] == pay
            pay_mod4.add((end - len(pay)) % 4)
    assert covered[8] == set(range(8, 16)) and covered[9] == set(range(9, 16)), covered
    assert len(pay_mod4) >= 3, pay_mod4

    def freqs(name):
        return walks[name]["freq"], walks[name]["cum"], cs[name]["pb"]

    # (a) every plane of the grey tile is one symbol: a stream of the initial state alone
    ta = dr.parse_tile(cs["a"]["tile"], 0, len(cs["a"]["tile"]), 256, 256)
    for L, half in zip(ta["layers"], (128, 256, 256)):
        assert L["pb"] is not None and len(L["stream"]) <= 29 and np.all(L["res"] == half)
    assert int(walks["a"]["freq"][128]) == 1 << 8 and walks["a"]["words"].size == 2
    # (b) 2^pb - 1 and 1
    for name in [n for n in cs if cs[n]["design"] == "b"]:
        f, _, pb = freqs(name)
        assert sorted(f[f > 0].tolist()) == [1, (1 << pb) - 1], name
    # (c), (d): groups at the ring bound of 8 words, none above it, long idle stretches; full buckets
    for name in ("c8", "d8", "c8_300", "burst9"):
        g = walks[name]["groups"]
        assert int((g == 8).sum()) >= 10 and int(g.max()) == 8, (name, np.bincount(g))
        assert int((g == 0).sum()) >= 1000, name
        assert 20 * 1024 < ds.BURST_AT < 21 * 1024 < ds.BURST_AT + 510
    for name, bottom, top in (("c8", True, False), ("d8", False, True), ("burst9", True, True),
                              ("c8_300", True, False)):
        f, cum, pb = freqs(name)
        per, _ = ds.bucket_starts(cum, pb)
        assert (per[0] == 64) == bottom and (per[-1] == 64) == top, (name, per[0], per[-1])
        if top:
            assert int(f[-1]) == 1 and int(cum[-1]) == 1 << pb   # the last start is slot 2^pb - 1
    assert int(walks["c8"]["freq"][255]) > 32000 and int(walks["d8"]["freq"][0]) > 32000
    # (e) equal frequencies 256 / 128: no start off a 64-slot edge
    for name, fq, cnt in (("e8", 256, 128), ("e9", 128, 256)):
        f, cum, pb = freqs(name)
        _, st = ds.bucket_starts(cum, pb)
        assert st.size == cnt and not np.any(st & 63) and set(f[f > 0].tolist()) == {fq}
    # (f) all 512 symbols
    for name in ("f", "f_300"):
        assert int((walks[name]["freq"] > 0).sum()) == 512
    # layouts: the 300 x 300 tiles end on a 912-symbol segment; the compacted planes
    assert cs["c8_300"]["res"].size % 1024 == 912
    n_small = dr.parse_tile(cs["lz_small"]["tile"], 0, len(cs["lz_small"]["tile"]), 256, 256)["layers"][0]["res"].size
    n_mid = dr.parse_tile(cs["lz_mid"]["tile"], 0, len(cs["lz_mid"]["tile"]), 256, 256)["layers"][0]["res"].size
    assert n_small < 1024 < n_mid < 16384 and n_small % 64 and n_mid % 64
    # a burst stream is the last stream of a file
    assert ds.FILES["F1"][2][-1] == "burst9" and cs["burst9"]["plane"] == 2
    assert all(max(W, H) <= 1024 and min(W, H) <= 512 for W, H, _ in ds.FILES.values())


def test_helper_reads_its_own_files():
    for name, (data, img, _) in ds.files().items():
        back, _ = dr.decode_file(data, img)
        assert np.array_equal(back, img), name


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def hoh():
    import torch  # noqa: F401  (before the first context: torch brings its own HIP runtime)
    import hoh_ans
    return hoh_ans


@pytest.fixture(scope="module")
def dev(hoh):
    """name -> (file on the device, size, image); the container is the library's own (build_file
    loads the library, which has to come after torch: checked here, not in the CPU tests)"""
    import torch
    cs = ds.cases()
    for d, img, offs in ds.files().values():
        assert d == dr.build_file(img.shape[1], img.shape[0], [cs[c]["tile"] for c, _ in offs])
    return {n: (torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda(), len(d), img)
            for n, (d, img, _) in ds.files().items()}


def _noix(hoh, mode):
    c = hoh.Context(0)
    c.set_option(hoh.OPT_NOIX_DECODER, {"lanes": hoh.NOIX_LANES, "multi": hoh.NOIX_MULTI, "wave": hoh.NOIX_WAVE,
                                        "adaptive": hoh.NOIX_ADAPTIVE}[mode])
    return c


def _wrong_tiles(name, got, img):
    """the cases whose tiles differ (for the assertion message)"""
    W, H, names = ds.FILES[name]
    return [c for (x0, y0, w, h), c in zip(dr.tile_rects(W, H), names)
            if not np.array_equal(got[y0:y0 + h, x0:x0 + w], img[y0:y0 + h, x0:x0 + w])]


def _decode(hoh, ctx, f, n, img, index, what):
    import torch
    H, W, _ = img.shape
    rgb, w, h = hoh.decode_image(f, n, ctx=ctx, index=index)
    torch.cuda.synchronize()
    assert (w, h) == (W, H)
    return rgb.cpu().numpy().reshape(H, W, 3)


@pytest.fixture(scope="module")
def built(hoh, dev):
    """name -> blob of the index hoh_index_build makes from the file alone (lanes chain)"""
    ctx = _noix(hoh, "lanes")
    out = {}
    for name, (f, n, _) in dev.items():
        ix = hoh.build_index(f, n, ctx=ctx)
        assert ix.nbytes() > 0
        out[name] = ix.to_bytes(ctx)
    ctx.close()
    return out


@gpu
@pytest.mark.parametrize("mode", NOIX)
def test_no_index_decode(hoh, dev, mode):
    ctx = _noix(hoh, mode)
    for name, (f, n, img) in dev.items():
        got = _decode(hoh, ctx, f, n, img, None, name)
        assert np.array_equal(got, img), (mode, name, _wrong_tiles(name, got, img))
    ctx.close()


@gpu
@pytest.mark.parametrize("name", list(ds.FILES))
def test_index_build(hoh, dev, name):
    f, n, img = dev[name]
    blobs = {}
    for kernel in ("lanes", "multi"):
        ctx = _noix(hoh, kernel)
        ix = hoh.build_index(f, n, ctx=ctx)
        blobs[kernel] = ix.to_bytes(ctx)
        assert len(blobs[kernel]) == ix.serialized_size() > 48
        if kernel == "lanes":                                 # the indexed decoder: k_drans's ring path
            got = _decode(hoh, ctx, f, n, img, ix, name)
            assert np.array_equal(got, img), (name, _wrong_tiles(name, got, img))
        ctx.close()
    assert blobs["lanes"] == blobs["multi"]
    fresh = hoh.Context(0)
    ix = hoh.Index.from_bytes(blobs["lanes"])
    assert ix.to_bytes() == blobs["lanes"]
    got = _decode(hoh, fresh, f, n, img, ix, name)
    assert np.array_equal(got, img), (name, _wrong_tiles(name, got, img))
    fresh.close()


@gpu
def test_built_index_drives_the_burst(hoh, dev, built):
    """the indexed decoder really starts the burst's segments from the built checkpoints: one bit of
    the checkpoint behind the burst's first segment (c8: G plane of F0's third tile) and the
    segment no longer meets it -- E_CORRUPT; the untouched blob decodes"""
    import struct
    f, n, img = dev["F0"]
    blob = built["F0"]
    ns, nck = struct.unpack_from("<I", blob, 12)[0], struct.unpack_from("<Q", blob, 32)[0]
    recs = [struct.unpack_from("<QIIII", blob, 48 + 24 * s) for s in range(ns)]
    assert ns == 7 * 8 and len(blob) == 48 + 24 * ns + 12 * nck
    g = 7 * ds.FILES["F0"][2].index("c8") + 3
    assert recs[g][1] == 65536 and recs[g][2] == 1
    first = sum((r[1] + 255) // 256 for r in recs[:g] if r[2] == 1)
    bad = bytearray(blob)
    bad[48 + 24 * ns + 12 * (first + ds.BURST_AT // 256 + 1)] ^= 0x10
    ctx = hoh.Context(0)
    with pytest.raises(hoh.HohError) as e:
        hoh.decode_image(f, n, ctx=ctx, index=hoh.Index.from_bytes(bytes(bad)))
    assert e.value.code == E_CORRUPT
    got = _decode(hoh, ctx, f, n, img, hoh.Index.from_bytes(blob), "F0")
    assert np.array_equal(got, img)
    ctx.close()


@gpu
@pytest.mark.parametrize("name", list(ds.FILES))
def test_region_decode(hoh, dev, built, name):
    import torch
    f, n, img = dev[name]
    x, y, w, h = ds.WINDOWS[name]
    tx0, ty0, ntx, nty = hoh.region_cover(img.shape[1], img.shape[0], x, y, w, h)
    assert ntx >= 2 and (nty >= 2 or img.shape[0] < 512)      # the window crosses a tile edge
    ctx = hoh.Context(0)
    for index in (None, hoh.Index.from_bytes(built[name])):
        win, W, H = hoh.decode_region(f, n, x, y, w, h, ctx=ctx, index=index)
        torch.cuda.synchronize()
        assert (H, W) == img.shape[:2]
        assert np.array_equal(win.cpu().numpy(), img[y:y + h, x:x + w]), (name, index is not None)
    ctx.close()


@gpu
def test_batched_decode(hoh, dev, built):
    import torch
    W, H, n = 1024, 512, len(BATCH)
    stride = (max(dev[b][1] for b in BATCH) + 101) | 1        # odd: every file at another alignment
    buf = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    for i, b in enumerate(BATCH):
        buf[i * stride:i * stride + dev[b][1]] = dev[b][0]
    want = np.stack([dev[b][2] for b in BATCH])
    ctx = hoh.Context(0)
    cat = hoh.Index.concat([hoh.Index.from_bytes(built[b]) for b in BATCH], stride)
    for index in (None, cat):
        dec = torch.zeros(n * W * H * 3, dtype=torch.uint8, device="cuda")
        st = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        hoh.decode_images_async(buf, n, stride, W, H, dec, st, ctx=ctx, index=index)
        torch.cuda.synchronize()
        s = st.cpu().numpy()
        for i in range(n):
            assert hoh.check_status(s[2 * i:2 * i + 2], "batch decode %d" % i) == W * H * 3
        got = dec.cpu().numpy().reshape(n, H, W, 3)
        for i, b in enumerate(BATCH):
            assert np.array_equal(got[i], want[i]), (b, index is not None, _wrong_tiles(b, got[i], want[i]))
    ctx.close()


def _one_stream(hoh, orc, ctx, sym, rng, pb, lead, what):
    """the stream behind `lead` bytes of something else: symbols and end pointer as the oracle's"""
    s = orc.encode_entropy(sym, rng, pb)
    buf = bytes(range(7, 7 + lead)) + s + b"\x5a\xa5\x5a"
    want, wend = orc.decode_entropy(buf, lead)
    assert wend == lead + len(s) and np.array_equal(want, sym)
    got, gend = hoh.decode_entropy(buf, lead, ctx=ctx)
    assert gend == wend and np.array_equal(np.asarray(got, np.uint16), want), what
    return s


@gpu
def test_single_streams(hoh, orc):
    ctx = hoh.Context(0)
    for k, (name, c) in enumerate(sorted(ds.cases().items())):
        if c["res"] is not None:
            s = _one_stream(hoh, orc, ctx, c["res"], 1 << c["depth"], c["pb"], k % 4, name)
            assert s[5] >> 7, name                            # (range, count: 2 + 3 varint bytes) rANS
    ctx.close()


# (range, prob_bits) at which the reference's encoder has no rANS stream that reads back: it takes
# the raw frequency table, whose fields are bitlen(range - 1) bits wide, for every histogram that
# is not stored, and the frequencies (sum 2^pb) do not fit them.  Checked over every
# split of 2^pb; here over the candidates below.
NO_RANS = {(2, 3), (2, 4), (2, 6), (3, 5)}
E_CORRUPT = 7


def _small_streams(orc):
    """ranges 2..64 at every prob_bits from the smallest that holds the range up to 6 ->
    [(range, prob_bits, symbols, stream)]: the first of a few skewed sequences (symbol 0 at 85 %,
    the rest geometric, cut at fewer and fewer symbols) whose stream is rANS and reads back -- near
    the smallest prob_bits only a table with a spare slot can favour a symbol, and a raw table
    holds only small frequencies.  The NO_RANS pairs keep their first rANS candidate."""
    rs = np.random.RandomState(6)
    out = []
    for rng in range(2, 65):
        for pb in range(max(1, int(rng - 1).bit_length()), 7):
            caps = sorted({rng - 1, min(rng - 1, (1 << pb) - 2), min(rng - 1, (1 << pb) // 2 - 1), 0}, reverse=True)
            keep = None
            for cap in caps:
                sym = np.minimum(rs.geometric(0.85, 1500) - 1, cap).astype(np.uint16)
                s = orc.encode_entropy(sym, rng, pb)
                if not s[3] >> 7:                             # (range: 1 byte, count: 2) stored
                    continue
                assert (s[3] & 0x7c) >> 2 == pb
                try:
                    back, end = orc.decode_entropy(s, 0)
                except orc.OracleError as e:
                    assert e.code == -5
                    keep = keep or (rng, pb, sym, s)
                    continue
                assert end == len(s) and np.array_equal(back, sym)
                assert (rng, pb) not in NO_RANS
                keep = (rng, pb, sym, s)
                break
            else:
                assert (rng, pb) in NO_RANS, (rng, pb)
            out.append(keep)
    return out


def test_small_prob_bits_inputs(orc):
    ss = _small_streams(orc)
    assert len(ss) == 120 and all(s is not None for s in ss)
    assert {(r, pb) for r, pb, _, _ in ss} == {(r, pb) for r in range(2, 65) for pb in range(1, 7) if 1 << pb >= r}


@gpu
def test_single_streams_small_prob_bits(hoh, orc):
    """prob_bits below the chain kernels' table format (>= 7): the plain path.  Symbols and end
    pointer are the oracle's; the four streams the oracle cannot read (NO_RANS: a table that does
    not sum to 2^pb) are E_CORRUPT here too."""
    ctx = hoh.Context(0)
    for k, (rng, pb, sym, s) in enumerate(_small_streams(orc)):
        if (rng, pb) in NO_RANS:
            with pytest.raises(hoh.HohError) as e:
                hoh.decode_entropy(bytes(k % 4) + s + b"\x5a\xa5\x5a", k % 4, ctx=ctx)
            assert e.value.code == E_CORRUPT, (rng, pb)
        else:
            assert _one_stream(hoh, orc, ctx, sym, rng, pb, k % 4, (rng, pb)) == s
    ctx.close()
