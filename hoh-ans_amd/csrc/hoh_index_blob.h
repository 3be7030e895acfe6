// Serialized side index (include/hoh_ans.h, hoh_index_serialize): layout constants and the
// validation of an untrusted blob.  Host only and free of HIP, so the parser also compiles into a
// stand-alone program (tools/index_blob_check.cpp) that runs under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define HOH_BLOB_VERSION 1u
#define HOH_BLOB_SEG 256u          // == HOH_SEG
#define HOH_BLOB_SPT 7u            // == SK_PER_TILE
#define HOH_BLOB_HDR 48u
#define HOH_BLOB_REC 24u
#define HOH_BLOB_CK 12u
#define HOH_BLOB_RANS 1u           // == SM_RANS (0 empty, 2 stored)

struct BlobHeader {
  uint32_t nstreams, nimg;
  uint64_t stride, nck;
};

static inline uint32_t blob_u32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
static inline uint64_t blob_u64(const uint8_t* p) { return (uint64_t)blob_u32(p) | (uint64_t)blob_u32(p + 4) << 32; }
static inline void blob_put32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}
static inline void blob_put64(uint8_t* p, uint64_t v) { blob_put32(p, (uint32_t)v); blob_put32(p + 4, (uint32_t)(v >> 32)); }

static inline const uint8_t* blob_rec(const uint8_t* blob, uint32_t s) { return blob + HOH_BLOB_HDR + (size_t)s * HOH_BLOB_REC; }
static inline const uint8_t* blob_ck(const uint8_t* blob, const BlobHeader& h, uint64_t k) {
  return blob + HOH_BLOB_HDR + (size_t)h.nstreams * HOH_BLOB_REC + (size_t)k * HOH_BLOB_CK;
}

// True when `blob` is a well-formed index of exactly `size` bytes (the checks listed in
// include/hoh_ans.h).  Every size is computed in 64 bits from fields already bounded by `size`,
// so nothing wraps: nstreams <= size / 24 and nck <= size / 12 before either is multiplied.
static inline bool blob_validate(const uint8_t* blob, size_t size, BlobHeader* out) {
  if (!blob || size < HOH_BLOB_HDR) return false;
  if (blob[0] != 'H' || blob[1] != 'O' || blob[2] != 'H' || blob[3] != 'X') return false;
  if (blob_u32(blob + 4) != HOH_BLOB_VERSION || blob_u32(blob + 8) != HOH_BLOB_SEG) return false;
  BlobHeader h;
  h.nstreams = blob_u32(blob + 12);
  h.nimg = blob_u32(blob + 16);
  h.stride = blob_u64(blob + 24);
  h.nck = blob_u64(blob + 32);
  if (blob_u32(blob + 20) != 0 || blob_u64(blob + 40) != 0) return false;
  if (h.nstreams % HOH_BLOB_SPT || h.nstreams > 0x7fffffffu) return false;
  if (h.nimg < 1 || h.nstreams % h.nimg) return false;
  if ((h.stride == 0) != (h.nimg == 1)) return false;
  const uint64_t body = (uint64_t)size - HOH_BLOB_HDR;
  if (h.nstreams > body / HOH_BLOB_REC) return false;
  const uint64_t rest = body - (uint64_t)h.nstreams * HOH_BLOB_REC;
  if (h.nck > rest / HOH_BLOB_CK || h.nck * HOH_BLOB_CK != rest) return false;
  if (h.nck > 0xffffffffull) return false;                  // checkpoint offsets are 32-bit
  uint64_t sum = 0;
  for (uint32_t s = 0; s < h.nstreams; s++) {
    const uint8_t* r = blob_rec(blob, s);
    const uint64_t off = blob_u64(r);
    const uint32_t n = blob_u32(r + 8), mode = blob_u32(r + 12), words = blob_u32(r + 16);
    if (mode > 2 || blob_u32(r + 20) != 0) return false;
    if (mode != HOH_BLOB_RANS) {
      if (off || n || words) return false;
      continue;
    }
    sum += ((uint64_t)n + HOH_BLOB_SEG - 1) / HOH_BLOB_SEG;   // < 2^24 each, 2^31 streams at most
  }
  if (sum != h.nck) return false;
  if (out) *out = h;
  return true;
}
