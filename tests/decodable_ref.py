"""A reader and a builder of .hoh files beyond the -s0 shape (predictor-map layers, 16-bit LZ
distances, RGB mode), made of oracle primitives only: decode_entropy / encode_entropy, a numpy LZ
walk (un_lz.hpp:150-170), unpredict_all / predict_all, add-green, or_find_lz_rgb, and
hoh_ans.file_prefix (host code) for the container.  The GPU encoder's decodable files are checked
against the reader, the GPU decoder against files of the builder."""
import ctypes as C

import numpy as np

MASKS = [0x0001, 0x0002, 0x0020, 0x0010, 0xffbf, 0x0003, 0xfffd, 0xfffb, 0xfff7, 0xffef, 0xffdf, 0xff7f,
         0xfdff, 0xffff]                                      # layer_encode.hpp:159-175


def _orc():
    import oracle
    return oracle


def rd_varint(b, p):
    b0 = b[p]; p += 1
    if not b0 & 0x80:
        return b0, p
    b1 = b[p]; p += 1
    if not b1 & 0x80:
        return ((b0 & 0x7f) << 7) + b1, p
    b2 = b[p]; p += 1
    return ((b0 & 0x7f) << 14) + ((b1 & 0x7f) << 7) + b2, p


def wr_varint(v):
    if v < 1 << 7:
        return bytes([v])
    if v < 1 << 14:
        return bytes([(v >> 7) + 128, v % 128])
    assert v < 1 << 21
    return bytes([(v >> 14) + 128, ((v >> 7) % 128) + 128, v % 128])


def tiles_of(data):
    """-> W, H, [(x0, y0, w, h, start, end)] of a tiled .hoh"""
    b = bytes(data)
    assert b[:6] == bytes([153, 72, 79, 72, 2, 8])
    p = 6
    W, p = rd_varint(b, p)
    H, p = rd_varint(b, p)
    W += 1; H += 1
    xt, yt = b[p] + 1, b[p + 1] + 1
    p += 2
    assert (xt, yt) == (W // 256, H // 256)
    n = xt * yt
    sizes = []
    for _ in range(n - 1):
        v, p = rd_varint(b, p)
        sizes.append(v)
    tw, th = (W + xt - 1) // xt, (H + yt - 1) // yt
    out = []
    for i in range(n):
        end = p + sizes[i] if i < n - 1 else len(b)
        x0, y0 = (i % xt) * tw, (i // xt) * th
        out.append((x0, y0, min(tw, W - x0), min(th, H - y0), p, end))
        p = end
    return W, H, out


def parse_tile(b, p, end, w, h):
    """The tile's parts: mode, LZ symbol streams, matches [(pos, len, back)], layers (grid, masks,
    map indices, residuals, prob_bits or None for a stored stream, and the residual stream's bytes)."""
    orc = _orc()
    b = bytes(b)
    assert b[p] == 0 and b[p + 1] == 0
    mode = b[p + 2]
    assert mode in (128, 2), mode
    assert b[p + 3] == 0x03
    q = p + 4
    lz = []
    for k in range(4):
        if k == 3 and b[q] == 0x24:
            break
        s, q = orc.decode_entropy(b[:end], q)
        lz.append(s.astype(np.int64))
    assert b[q] == 0x24
    q += 1
    L1, q = rd_varint(b, q)
    L2, q = rd_varint(b, q)
    starts = [q, q + L1, q + L1 + L2]
    fut, ln, bb = lz[0], lz[1], lz[2]
    bb2 = lz[3] if len(lz) == 4 else np.zeros_like(bb)
    matches = []
    idx = g = 0
    for v in fut:
        idx += int(v)
        if v == 255:
            continue
        L = int(ln[g]) + 4
        matches.append((idx, L, int(bb[g]) | (int(bb2[g]) << 8)))
        idx += L
        g += 1
    assert idx <= w * h and g == len(ln) == len(bb)
    layers = []
    for k, s in enumerate(starts):
        assert b[s] == 0x10, hex(b[s])
        xt, yt = b[s + 1] + 1, b[s + 2] + 1
        if xt == 1 and yt == 1:
            masks = [(b[s + 3] << 8) | b[s + 4]]
            pidx = np.zeros(1, np.uint16)
            r = s + 5
            mapped = False
        else:
            nm = b[s + 3]
            assert 1 <= nm <= 16
            masks = [(b[s + 4 + 2 * i] << 8) | b[s + 5 + 2 * i] for i in range(nm)]
            pidx, r = orc.decode_entropy(b[:end], s + 4 + 2 * nm)
            assert pidx.size == xt * yt and int(pidx.max()) < nm
            mapped = True
        _, vp = rd_varint(b, r)
        _, vp = rd_varint(b, vp)
        meta = b[vp]
        pb = (meta & 0x7c) >> 2 if meta >> 7 else None
        lim = starts[k + 1] if k < 2 else end
        if pb is not None and pb > 15:
            # prob_bits 16..19 carry into bit 6 of the metadata byte (entropy_encoding.hpp:138), which
            # the oracle's reader masks off like the reference's: such a stream is taken whole, and
            # decode_tile checks it against the encoding of the residuals the pixels imply
            res, e = None, lim
        else:
            res, e = orc.decode_entropy(b[:end], r)
        assert e == lim, (k, e, lim)                            # nothing clipped, nothing left over
        layers.append(dict(xt=xt, yt=yt, masks=masks, pidx=pidx, mapped=mapped, res=res, pb=pb, stream=b[r:e]))
    return dict(mode=mode, nlz=len(lz), matches=matches, layers=layers)


def backref_of(matches, npix):
    br = np.zeros(npix, np.uint16)
    for pos, L, back in matches:
        assert 0 < back <= pos, (pos, L, back)
        br[pos:pos + L] = back
    return br


def decode_tile(b, p, end, w, h, orig=None):
    """orig: the tile's true pixels, needed only for residual streams at prob_bits 16..19 (see
    parse_tile): their residuals are recomputed from orig and must encode to the stream's bytes."""
    orc = _orc()
    t = parse_tile(b, p, end, w, h)
    br = backref_of(t["matches"], w * h)
    planes = []
    for k, L in enumerate(t["layers"]):
        depth = 9 if (k and t["mode"] == 128) else 8
        tm = np.array([L["masks"][i] for i in L["pidx"]], np.uint16)
        if L["res"] is None:
            assert orig is not None, "a prob_bits %d stream needs the original pixels" % L["pb"]
            o = np.asarray(orig).astype(np.int64)
            g = o[..., 1]
            pl = g if k == 0 else o[..., 0 if k == 1 else 2] + ((256 - g) if t["mode"] == 128 else 0)
            L["res"] = orc.predict_all(pl.astype(np.uint16), depth, L["xt"], L["yt"], tm)[br == 0]
            assert orc.encode_entropy(L["res"], 1 << depth, L["pb"]) == L["stream"], (k, L["pb"])
        assert L["res"].size == int((br == 0).sum())
        if not L["mapped"] and L["masks"] == [0x0010]:         # the -s0 layer: MED on every row
            pl = orc.unpredict_fastpath(L["res"], w, h, depth, br if br.any() else None)
        else:
            pl = orc.unpredict_all(L["res"], w, h, depth, L["xt"], L["yt"], tm, br if br.any() else None)
        planes.append(pl.astype(np.int64))
    g, r, bl = planes
    if t["mode"] == 128:
        r, bl = r + g - 256, bl + g - 256
    return np.stack([r, g, bl], -1).astype(np.uint8), t


def decode_file(data, orig=None):
    """-> (image, [parsed tiles])"""
    W, H, tiles = tiles_of(data)
    img = np.zeros((H, W, 3), np.uint8)
    parsed = []
    for x0, y0, w, h, s, e in tiles:
        px, t = decode_tile(data, s, e, w, h, None if orig is None else orig[y0:y0 + h, x0:x0 + w])
        img[y0:y0 + h, x0:x0 + w] = px
        parsed.append(t)
    return img, parsed


def ladder_pb(res, rng):
    """the decodable ladder: candidates 16..19 if s(16) < s(15) else 15..12, first of strictly
    smallest size -> (prob_bits, stream)"""
    orc = _orc()
    s = {pb: orc.encode_entropy(res, rng, pb) for pb in (16, 15)}
    cand = [16, 17, 18, 19] if len(s[16]) < len(s[15]) else [15, 14, 13, 12]
    best = None
    for pb in cand:
        e = s.get(pb) or orc.encode_entropy(res, rng, pb)
        if best is None or len(e) < len(best[1]):
            best = (pb, e)
    return best


def find_lz(tile, distance, bonus=0):
    """or_find_lz_rgb -> (LZ bytes: 0x03 + 3 streams, 4 if distance > 8; nuke map)"""
    orc = _orc()
    L = orc.lib()
    px = np.ascontiguousarray(tile, np.uint8)
    h, w, _ = px.shape
    out = np.empty(4 * (w * h + 4096) + 4096, np.uint8)
    nuke = np.zeros(w * h, np.uint8)
    u8p = C.POINTER(C.c_uint8)
    n = L.or_find_lz_rgb(px.ctypes.data_as(u8p), px.size, w, h, out.ctypes.data_as(u8p), nuke.ctypes.data_as(u8p),
                         distance, bonus)
    assert n > 0
    return out[:n].tobytes(), nuke


def build_tile(tile, layers, mode=128, lz_distance=None, pbs=(15, 15, 15)):
    """One tile's bytes.  layers: three (xt, yt, masks, pidx) -- pidx indexes masks per grid cell;
    a 1x1 grid writes masks[0] alone.  lz_distance None: no copies (three empty streams)."""
    orc = _orc()
    px = np.ascontiguousarray(tile, np.uint8)
    h, w, _ = px.shape
    if lz_distance is None:
        lzb, nuke = bytes([0x03]) + orc.encode_entropy(np.zeros(0, np.uint16), 256, 10) * 3, np.zeros(w * h, np.uint8)
    else:
        lzb, nuke = find_lz(px, lz_distance)
    r, g, b = (px[..., i].astype(np.int64) for i in range(3))
    planes = [g, r - g + 256, b - g + 256] if mode == 128 else [g, r, b]
    lay = []
    for k, (xt, yt, masks, pidx) in enumerate(layers):
        depth = 9 if (k and mode == 128) else 8
        pidx = np.asarray(pidx, np.uint16)
        tm = np.array([masks[i] for i in pidx], np.uint16)
        if xt == 1 and yt == 1 and masks[0] == 0x0010:         # the -s0 layer: MED on every row, as decode_tile reads it
            res = orc.predict_fastpath(planes[k].astype(np.uint16), depth).reshape(-1)[nuke == 0]
        else:
            res = orc.predict_all(planes[k].astype(np.uint16), depth, xt, yt, tm)[nuke == 0]
        if xt == 1 and yt == 1:
            hdr = bytes([0x10, 0, 0, masks[0] >> 8, masks[0] & 255])
        else:
            hdr = bytes([0x10, xt - 1, yt - 1, len(masks)]) + b"".join(bytes([m >> 8, m & 255]) for m in masks)
            hdr += orc.encode_entropy(pidx, len(masks), 8)
        lay.append(hdr + orc.encode_entropy(res, 1 << depth, pbs[k]))
    return (bytes([0, 0, mode]) + lzb + bytes([0x24]) + wr_varint(len(lay[0])) + wr_varint(len(lay[1])) +
            lay[0] + lay[1] + lay[2])


def build_file(W, H, tiles):
    import hoh_ans
    return hoh_ans.file_prefix(W, H, [len(t) for t in tiles]) + b"".join(tiles)


def tile_rects(W, H):
    xt, yt = W // 256, H // 256
    tw, th = (W + xt - 1) // xt, (H + yt - 1) // yt
    return [((i % xt) * tw, (i // xt) * th, min(tw, W - (i % xt) * tw), min(th, H - (i // xt) * th))
            for i in range(xt * yt)]
