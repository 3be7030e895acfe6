"""The serialized side index (include/hoh_ans.h, hoh_index_serialize) is untrusted input to
hoh_index_deserialize: every structural violation must read as HOH_E_CORRUPT, on the host, before
any device call -- so this runs without a GPU (hoh_index_create needs none).  The blob below is
built with struct.pack from the layout documented in the header, not by the library."""
import ctypes as C
import struct

import pytest

import hoh_ans

SEG = 256
RANS, STORED, EMPTY = 1, 2, 0
E_ARG, E_HIP, E_CORRUPT, E_NODEV = 1, 3, 7, 8


def _tile(base):
    """seven stream records of one tile: (payload_off, n, mode, words)"""
    return [(base + 40, 300, RANS, 90), (0, 0, STORED, 0), (0, 0, EMPTY, 0),
            (base + 500, 65536, RANS, 20000), (base + 90000, 65536, RANS, 21000), (base + 180000, 65536, RANS, 22000),
            (0, 0, EMPTY, 0)]


def make_blob(recs=None, nimg=1, stride=0, nck=None, magic=b"HOHX", version=1, seg=SEG, nstreams=None, res0=0, res1=0):
    recs = list(recs if recs is not None else _tile(20) + _tile(300000))
    total = sum((n + SEG - 1) // SEG for _, n, m, _ in recs if m == RANS)
    nck = total if nck is None else nck
    b = magic + struct.pack("<IIIIIQQQ", version, seg, len(recs) if nstreams is None else nstreams, nimg, res0, stride,
                            nck, res1)
    for off, n, mode, words in recs:
        b += struct.pack("<QIIII", off, n, mode, words, 0)
    for k in range(total):
        b += struct.pack("<III", 0x1234 + k, 0x80000000 | k, 2 + 3 * k)
    return b


def _load(blob):
    L = hoh_ans.lib()
    h = C.c_void_p()
    assert L.hoh_index_create(C.byref(h)) == 0
    try:
        r = L.hoh_index_deserialize(h, bytes(blob), len(blob), None)
        return r, L.hoh_index_bytes(h), L.hoh_index_serialized_size(h) if r else None
    finally:
        L.hoh_index_destroy(h)


def _recs_with(i, rec):
    r = _tile(20) + _tile(300000)
    r[i] = rec
    return r


GOOD = make_blob()
MUTATIONS = {
    "one byte cut off": GOOD[:-1],
    "one byte appended": GOOD + b"\0",
    "wrong magic": make_blob(magic=b"HOHY"),
    "version 2": make_blob(version=2),
    "seg 128": make_blob(seg=128),
    "nstreams 13": make_blob(nstreams=13),
    "nimg 0": make_blob(nimg=0),
    "nimg 1 with stride 8": make_blob(nimg=1, stride=8),
    "nimg 2 with stride 0": make_blob(nimg=2, stride=0),
    "mode 3": make_blob(recs=_recs_with(2, (0, 0, 3, 0))),
    "words in a stored record": make_blob(recs=_recs_with(1, (0, 0, STORED, 5))),
    "n raised by 256, nck kept": GOOD[:48 + 3 * 24 + 8] + struct.pack("<I", 65536 + 256) + GOOD[48 + 3 * 24 + 12:],
    "nck 2**63": GOOD[:32] + struct.pack("<Q", 2 ** 63) + GOOD[40:],
    "reserved header word": make_blob(res0=1),
    "reserved header tail": make_blob(res1=1),
    "header cut short": GOOD[:47],
    "empty": b"",
}


def test_layout_of_the_test_blob():
    assert len(GOOD) == 48 + 14 * 24 + 12 * 2 * (2 + 3 * 256)
    assert len(MUTATIONS["n raised by 256, nck kept"]) == len(GOOD)
    assert len(MUTATIONS["nck 2**63"]) == len(GOOD)


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_malformed_blob_is_corrupt(name):
    r, nbytes, ssize = _load(MUTATIONS[name])
    assert r == E_CORRUPT, name
    assert nbytes == 0 and ssize == 48, "a failed load leaves the empty index"


def test_wellformed_blob_passes_validation():
    """without a GPU the upload fails (E_HIP / E_NODEV); with one the load succeeds"""
    r, _, _ = _load(GOOD)
    assert r not in (E_CORRUPT, E_ARG)
    assert r in (0, E_HIP, E_NODEV)


def test_empty_index_is_its_header():
    L = hoh_ans.lib()
    h = C.c_void_p()
    assert L.hoh_index_create(C.byref(h)) == 0
    n = C.c_size_t(0)
    assert L.hoh_index_serialize(h, None, 0, C.byref(n), None) == 2 and n.value == 48      # E_CAP, size needed
    buf = (C.c_uint8 * 48)()
    assert L.hoh_index_serialize(h, buf, 48, C.byref(n), None) == 0 and n.value == 48
    want = b"HOHX" + struct.pack("<IIIIIQQQ", 1, SEG, 0, 1, 0, 0, 0, 0)
    assert bytes(buf) == want
    assert L.hoh_index_deserialize(h, want, 48, None) == 0                                 # no device needed
    assert L.hoh_index_bytes(h) == 0
    L.hoh_index_destroy(h)
