"""CPU self-test of tests/decodable_ref.py: a 2-tile file of its builder (random predictor maps, a
non-40-px grid, 4-stream LZ, RGB mode) read back by its own reader."""
import numpy as np

import decodable_ref as dr


def _image(rs, W, H):
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(x * 2 + y) // 3, (x + y * 3) // 5, (x * y) // 97], -1) + rs.randint(-3, 4, (H, W, 3))
    img = (img % 256).astype(np.uint8)
    img[40:47] = img[20:27]                                   # copies seven rows up
    img[100, 30:200] = img[99, 30:200]
    return img


def test_builder_reader_round_trip(orc):
    rs = np.random.RandomState(5)
    W, H = 512, 256
    img = _image(rs, W, H)
    tiles = []
    for k, (x0, y0, w, h) in enumerate(dr.tile_rects(W, H)):
        px = img[y0:y0 + h, x0:x0 + w]
        xt, yt = (7, 7) if k == 0 else (5, 9)
        masks = dr.MASKS[:4] + [0x1234] if k == 0 else [dr.MASKS[4], dr.MASKS[13]]
        layers = [(xt, yt, masks, rs.randint(0, len(masks), xt * yt)) for _ in range(3)]
        tiles.append(dr.build_tile(px, layers, mode=128 if k == 0 else 2, lz_distance=10, pbs=(15, 12, 16)))
    data = dr.build_file(W, H, tiles)
    back, parsed = dr.decode_file(data, img)
    assert np.array_equal(back, img)
    assert [t["mode"] for t in parsed] == [128, 2]
    assert all(t["nlz"] == 4 and t["matches"] for t in parsed)
    assert [L["pb"] for L in parsed[0]["layers"]] == [15, 12, 16]
