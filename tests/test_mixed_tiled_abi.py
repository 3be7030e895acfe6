"""CPU: hoh_mixed_rgb_bytes for the shapes the mixed calls take since tiled images joined the small
class -- every shape hoh_tiling tiles, in any mix with small ones; 64-bit offsets; the remaining
untiled shapes (one side under 256, the other 512 or more) still refused with nothing written."""
import ctypes as C

import pytest

from test_mixed_abi import raw


@pytest.fixture(scope="module")
def hoh():
    import hoh_ans
    hoh_ans.lib()
    return hoh_ans


def test_hand_computed_tiled(hoh):
    shapes = [(512, 256), (64, 48), (513, 257), (300, 512)]
    # 393216, 9216, 395523, 460800 bytes
    want = [0, 393216, 402432, 797955, 1258755]
    assert raw(hoh, shapes) == (1258755, want)
    assert raw(hoh, shapes, offsets=False)[0] == 1258755
    assert hoh.mixed_rgb_bytes(shapes) == (1258755, want)
    assert hoh.mixed_rgb_bytes([(256, 512)]) == (393216, [0, 393216])


def test_offsets_past_32_bits(hoh):
    one = 3 * 8192 * 8192                                          # 201326592
    total, off = hoh.mixed_rgb_bytes([(8192, 8192)] * 30 + [(64, 48)])
    assert one * 22 > 1 << 32
    assert off == [one * i for i in range(31)] + [one * 30 + 9216]
    assert total == one * 30 + 9216 == 6039806976


def test_untiled_wide_still_refused(hoh):
    for bad in ((512, 10), (10, 512), (255, 512), (1024, 255)):
        total, off = raw(hoh, [(512, 256), bad, (9, 9)])
        assert total == 0 and off == [0xDEAD] * 4, bad           # nothing written
        with pytest.raises(hoh.HohError) as e:
            hoh.mixed_rgb_bytes([(512, 256), bad])
        assert e.value.code == 1
    assert hoh.lib().hoh_mixed_rgb_bytes(1, (C.c_int32 * 2)(512, 0), None) == 0


def test_index_calls_exported(hoh):
    """the per-file persistence calls of a batch index with unequal tile counts"""
    L = hoh.lib()
    assert hasattr(L, "hoh_index_file") and hasattr(L, "hoh_index_join")
    assert L.hoh_index_file(None, 0, None, None) == 1
    assert L.hoh_index_join(None, 1, None, 0, None) == 1
