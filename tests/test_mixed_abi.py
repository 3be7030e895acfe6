"""CPU: hoh_mixed_rgb_bytes, the host-only helper of the mixed-shape batch calls -- the packed
layout (image i at the sum of 3 * W * H before it) and its argument checks.  tests/test_abi.py
covers the exported symbols."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def hoh():
    import hoh_ans
    hoh_ans.lib()
    return hoh_ans


def raw(hoh, shapes, n=None, offsets=True):
    flat = [v for p in shapes for v in p]
    wh = (C.c_int32 * max(len(flat), 1))(*flat)
    n = len(shapes) if n is None else n
    off = (C.c_uint64 * (max(n, 0) + 1))(*([0xDEAD] * (max(n, 0) + 1)))
    total = hoh.lib().hoh_mixed_rgb_bytes(n, wh, off if offsets else None)
    return int(total), [int(v) for v in off]


def test_hand_computed(hoh):
    shapes = [(1, 1), (511, 511), (63, 65), (2, 7), (300, 16)]
    # 3, 783363, 12285, 42, 14400 bytes
    want = [0, 3, 783366, 795651, 795693, 810093]
    assert raw(hoh, shapes) == (810093, want)
    assert raw(hoh, shapes, offsets=False)[0] == 810093           # offsets may be NULL
    assert hoh.mixed_rgb_bytes(shapes) == (810093, want)
    assert hoh.mixed_rgb_bytes([(224, 224)]) == (150528, [0, 150528])
    # the largest batch: 256 images of 511 x 511 (the sum needs more than 27 bits)
    total, off = hoh.mixed_rgb_bytes([(511, 511)] * 256)
    assert total == 256 * 783363 and off[255] == 255 * 783363


def test_refusals(hoh):
    assert hoh.lib().hoh_mixed_rgb_bytes(0, (C.c_int32 * 2)(4, 4), None) == 0
    assert raw(hoh, [(4, 4)] * 257)[0] == 0
    assert hoh.lib().hoh_mixed_rgb_bytes(1, None, None) == 0
    for bad in ((512, 10), (10, 512), (0, 5), (5, -1)):
        total, off = raw(hoh, [(8, 8), bad, (9, 9)])
        assert total == 0 and off == [0xDEAD] * 4, bad           # nothing written
    for shapes in ([], [(4, 4)] * 257, [(8, 8), (512, 10)]):
        with pytest.raises(hoh.HohError) as e:
            hoh.mixed_rgb_bytes(shapes)
        assert e.value.code == 1
