// Mixed-shape batches of small images (hoh_encode_mixed_async / hoh_decode_mixed_async): the front
// and the back of a job whose n tiles have n shapes.  The encoder (k_front.hip .. k_assemble.hip)
// and the decoder proper (k_decode.hip) run on a staging surface of one pitch in between: image i
// is the w_i x h_i tile at (0, i * hmax) of an xt = 1, yt = n stack of wmax x hmax slabs.
//  k_mgather:  the caller's packed images (image i at the sum of 3 * w * h before it) -> the
//              encoder's staging surface.
//  k_mheader:  each file's own header (8, 9 or 10 bytes: the varints of W - 1 and H - 1 change
//              length at 128) at i * stride.
//  k_dmixed:   the decoder's front, one wave per file: checks file i's header against (w_i, h_i)
//              and writes its DecTile (instead of k_dhdr + k_dtable: one tile per file, no table).
//  k_mscatter: the decoder's staging surface -> the caller's packed images.
//  k_mstatus_dec: {status, w_i * h_i * 3} per image.
#include "hoh_dec.h"
#include "hoh_rowmove.h"

// All of these are bound by memory latency / bandwidth and tiny beside the coding: no LDS, no
// barriers, one wave per unit of work.

// byte offset of image f in the packed buffer: a prefix over at most 256 products (<= 256 * 511 *
// 511 * 3 < 2^28), by every lane of a wave
__device__ __forceinline__ uint32_t mixed_off(const MixedDims& d, int f, int lane) {
  uint32_t v = 0;
  for (int k = lane; k < f; k += 64) v += 3u * (uint32_t)d.wh[2 * k] * (uint32_t)d.wh[2 * k + 1];
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One wave per image row (wave_move_row).  The gather reads the CALLER's buffer: every load of the
// mover is a byte of the row or an aligned dword / uint4 holding at least one byte of it, so none
// leaves the caller's allocation.  The scatter writes only image f's bytes (neighbouring images
// share dwords: byte heads and tails) and nothing at all after a failed decode.
#define MIX_ROWS 4       // rows (waves) per workgroup
__global__ __launch_bounds__(64 * MIX_ROWS) void k_mgather(MixedDims d, const uint8_t* packed, uint8_t* stage) {
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const int r = blockIdx.x * MIX_ROWS + (threadIdx.x >> 6);
  const int w = d.wh[2 * f], h = d.wh[2 * f + 1];
  if (r >= h) return;                                         // wave-uniform
  const uint32_t nb = (uint32_t)w * 3;
  const uint8_t* s = packed + (size_t)mixed_off(d, f, lane) + (size_t)r * nb;
  uint8_t* o = stage + ((size_t)f * d.hmax + r) * d.pitch * 3;
  wave_move_row(s, o, nb, lane);
}

__global__ __launch_bounds__(64 * MIX_ROWS) void k_mscatter(MixedDims d, const uint8_t* stage, uint8_t* packed,
                                                            const uint32_t* gerr) {
  if (*(volatile const uint32_t*)gerr) return;               // a failed decode leaves the caller's buffer alone
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const int r = blockIdx.x * MIX_ROWS + (threadIdx.x >> 6);
  const int w = d.wh[2 * f], h = d.wh[2 * f + 1];
  if (r >= h) return;
  const uint32_t nb = (uint32_t)w * 3;
  const uint8_t* s = stage + ((size_t)f * d.hmax + r) * d.pitch * 3;
  uint8_t* o = packed + (size_t)mixed_off(d, f, lane) + (size_t)r * nb;
  wave_move_row(s, o, nb, lane);
}

// a file whose stride cannot hold its header gets nothing (its status is HOH_E_CAP: k_layout counts
// the header into the file's size)
__global__ void k_mheader(MixedDims d, uint8_t* out, uint64_t stride) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.n) return;
  uint8_t hb[12];
  const uint32_t hl = mixed_hdr_bytes(d, i, hb);
  if (hl > stride) return;
  uint8_t* o = out + (uint64_t)i * stride;
#pragma unroll
  for (uint32_t k = 0; k < 10; k++)
    if (k < hl) o[k] = hb[k];
}

__global__ __launch_bounds__(64) void k_dmixed(MixedDims d, const uint8_t* in, uint64_t size, uint64_t stride,
                                               DecTile* tiles, uint32_t* gerr) {
  const int f = blockIdx.x, lane = threadIdx.x;
  uint8_t hb[12];
  const uint32_t hl = mixed_hdr_bytes(d, f, hb);
  uint64_t lo = 0, hi = 0;
#pragma unroll
  for (uint32_t k = 0; k < 10; k++) {
    const uint64_t b = k < hl ? hb[k] : 0;
    if (k < 8) lo |= b << (8 * k); else hi |= b << (8 * (k - 8));
  }
  // every read of file f stays inside [f * stride, (f + 1) * stride)
  const uint64_t base = (uint64_t)f * stride;
  const uint64_t fend = min(size, base + stride);
  bool bad = base + hl > fend;
  if (!bad && (uint32_t)lane < hl) {
    const uint8_t want = (uint8_t)((lane < 8 ? lo >> (8 * lane) : hi >> (8 * (lane - 8))) & 255);
    bad = in[base + lane] != want;
  }
  if (__any(bad) && lane == 0) atomicOr(gerr, 1u);
  if (lane == 0) {
    DecTile t;
    t.x0 = 0;
    t.y0 = f * d.hmax;
    t.w = d.wh[2 * f];
    t.h = d.wh[2 * f + 1];
    t.off = base + hl;
    t.mode = 0; t.nmatch = 0; t.err = 0; t.gen = 0;
    tiles[f] = t;
  }
}

// decoder error word -> {HOH status code, decoded bytes} per image: the job's error word for all
__global__ void k_mstatus_dec(MixedDims d, const uint32_t* gerr, uint64_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.n) return;
  const uint32_t g = gerr[0];
  out[2 * i] = g ? ((g & 2) ? 6 : 7) : 0;
  out[2 * i + 1] = g ? 0 : 3ull * (uint64_t)d.wh[2 * i] * (uint64_t)d.wh[2 * i + 1];
}

void launch_mgather(const MixedDims& d, const uint8_t* packed, uint8_t* stage, hipStream_t s) {
  hipLaunchKernelGGL(k_mgather, dim3((d.hmax + MIX_ROWS - 1) / MIX_ROWS, d.n), dim3(64 * MIX_ROWS), 0, s, d, packed, stage);
}

void launch_mscatter(const MixedDims& d, const uint8_t* stage, uint8_t* packed, const uint32_t* gerr, hipStream_t s) {
  hipLaunchKernelGGL(k_mscatter, dim3((d.hmax + MIX_ROWS - 1) / MIX_ROWS, d.n), dim3(64 * MIX_ROWS), 0, s, d, stage, packed,
                     gerr);
}

void launch_mheader(const MixedDims& d, uint8_t* out, uint64_t stride, hipStream_t s) {
  hipLaunchKernelGGL(k_mheader, dim3((d.n + 63) / 64), dim3(64), 0, s, d, out, stride);
}

void launch_dmixed(const MixedDims& d, const uint8_t* in, uint64_t size, uint64_t stride, DecTile* tiles,
                   uint32_t* gerr, hipStream_t s) {
  hipLaunchKernelGGL(k_dmixed, dim3(d.n), dim3(64), 0, s, d, in, size, stride, tiles, gerr);
}

void launch_mstatus_dec(const MixedDims& d, const uint32_t* gerr, uint64_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_mstatus_dec, dim3((d.n + 63) / 64), dim3(64), 0, s, d, gerr, out);
}
