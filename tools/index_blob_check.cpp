// Stand-alone check of the side-index blob parser (hoh-ans_amd/csrc/hoh_index_blob.h) for the host
// sanitizers: the parser is plain C++ with no HIP, so it builds with any compiler,
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o index_blob_check tools/index_blob_check.cpp && ./index_blob_check
// It feeds blob_validate the two-tile blob of tests/test_index_blob.py, each of that test's
// mutations, every truncation of the blob and a few thousand single-byte edits, each from a heap
// buffer of exactly the blob's size (so a read past the end is an AddressSanitizer report), and
// walks the records and checkpoints of every blob that validates, as hoh_index_deserialize does.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../hoh-ans_amd/csrc/hoh_index_blob.h"

typedef std::vector<uint8_t> Blob;
struct Rec { uint64_t off; uint32_t n, mode, words; };

static void p32(Blob& b, uint32_t v) { for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * i))); }
static void p64(Blob& b, uint64_t v) { p32(b, (uint32_t)v); p32(b, (uint32_t)(v >> 32)); }

static std::vector<Rec> tiles() {
  std::vector<Rec> r;
  for (uint64_t base : {20ull, 300000ull}) {
    r.push_back({base + 40, 300, 1, 90});
    r.push_back({0, 0, 2, 0});
    r.push_back({0, 0, 0, 0});
    r.push_back({base + 500, 65536, 1, 20000});
    r.push_back({base + 90000, 65536, 1, 21000});
    r.push_back({base + 180000, 65536, 1, 22000});
    r.push_back({0, 0, 0, 0});
  }
  return r;
}

static Blob make(const std::vector<Rec>& recs, uint32_t nimg = 1, uint64_t stride = 0, const char* magic = "HOHX",
                 uint32_t version = 1, uint32_t seg = 256, int nstreams = -1) {
  uint64_t total = 0;
  for (const Rec& r : recs) if (r.mode == 1) total += (r.n + 255) / 256;
  Blob b(magic, magic + 4);
  p32(b, version); p32(b, seg); p32(b, nstreams < 0 ? (uint32_t)recs.size() : (uint32_t)nstreams); p32(b, nimg); p32(b, 0);
  p64(b, stride); p64(b, total); p64(b, 0);
  for (const Rec& r : recs) { p64(b, r.off); p32(b, r.n); p32(b, r.mode); p32(b, r.words); p32(b, 0); }
  for (uint64_t k = 0; k < total; k++) { p32(b, 0x1234 + (uint32_t)k); p32(b, 0x80000000u | (uint32_t)k); p32(b, 2 + 3 * (uint32_t)k); }
  return b;
}

// validate from an exact-size heap copy; walk what a loader reads when it passes
static bool check(const Blob& b, uint64_t* sink) {
  uint8_t* h = new uint8_t[b.size() ? b.size() : 1];
  if (!b.empty()) memcpy(h, b.data(), b.size());
  BlobHeader bh;
  const bool ok = blob_validate(h, b.size(), &bh);
  if (ok) {
    for (uint32_t s = 0; s < bh.nstreams; s++) *sink += blob_u64(blob_rec(h, s)) + blob_u32(blob_rec(h, s) + 20);
    for (uint64_t k = 0; k < bh.nck; k++) *sink += blob_u32(blob_ck(h, bh, k) + 8);
  }
  delete[] h;
  return ok;
}

int main() {
  uint64_t sink = 0;
  int bad = 0;
  const Blob good = make(tiles());
  auto expect = [&](const char* name, const Blob& b, bool want) {
    const bool got = check(b, &sink);
    if (got != want) { std::printf("FAIL %s: validates %d, expected %d\n", name, (int)got, (int)want); bad++; }
  };
  expect("good", good, true);
  { Blob b = good; b.pop_back(); expect("one byte cut off", b, false); }
  { Blob b = good; b.push_back(0); expect("one byte appended", b, false); }
  expect("wrong magic", make(tiles(), 1, 0, "HOHY"), false);
  expect("version 2", make(tiles(), 1, 0, "HOHX", 2), false);
  expect("seg 128", make(tiles(), 1, 0, "HOHX", 1, 128), false);
  expect("nstreams 13", make(tiles(), 1, 0, "HOHX", 1, 256, 13), false);
  expect("nimg 0", make(tiles(), 0), false);
  expect("nimg 1 with stride 8", make(tiles(), 1, 8), false);
  expect("nimg 2 with stride 0", make(tiles(), 2, 0), false);
  expect("nimg 2 with a stride", make(tiles(), 2, 400000), true);
  { auto r = tiles(); r[2].mode = 3; expect("mode 3", make(r), false); }
  { auto r = tiles(); r[1].words = 5; expect("words in a stored record", make(r), false); }
  { Blob b = good; const uint32_t n = 65536 + 256; memcpy(&b[48 + 3 * 24 + 8], &n, 4); expect("n raised by 256", b, false); }
  { Blob b = good; const uint64_t v = 1ull << 63; memcpy(&b[32], &v, 8); expect("nck 2^63", b, false); }
  { Blob b = good; const uint64_t v = ~0ull / 12 + 1; memcpy(&b[32], &v, 8); expect("nck * 12 wraps", b, false); }
  { Blob b = good; const uint32_t v = 0xfffffff9u; memcpy(&b[12], &v, 4); expect("nstreams 2^32 - 7", b, false); }
  { Blob b = good; b[20] = 1; expect("reserved word", b, false); }
  { Blob b = good; b[47] = 1; expect("reserved tail", b, false); }
  expect("empty index", make({}), true);
  expect("no bytes", Blob(), false);
  // every truncation
  for (size_t n = 0; n < good.size(); n += n < 512 ? 1 : 97) expect("truncation", Blob(good.begin(), good.begin() + n), false);
  // single-byte edits of the header and the records: must not read out of bounds, whatever they return
  uint32_t rng = 12345;
  for (int it = 0; it < 4000; it++) {
    rng = rng * 1664525u + 1013904223u;
    Blob b = good;
    b[(rng >> 8) % (48 + 14 * 24)] ^= (uint8_t)(1u << (rng & 7));
    (void)check(b, &sink);
  }
  std::printf("%s (%d failures, sink %llu)\n", bad ? "index blob check FAILED" : "index blob check ok", bad,
              (unsigned long long)sink);
  return bad ? 1 : 0;
}
