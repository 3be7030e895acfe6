// Region decode (hoh_decode_region*): the front and the back of a decode job that restores only
// the tiles a pixel window touches.  The decoder proper (k_decode.hip) runs unchanged on the short
// tile list in between.
//  k_dregion: after k_dtable has turned the whole tile table of every file into byte offsets (a
//             prefix sum, so the table is read whole), one workgroup per file writes a DecTile for
//             each tile of its window's cover -- offset from the table, size from the file's
//             geometry, position inside the file's slab of the staging surface -- and the tile's
//             number in the side index's numbering (gid = file * file_tiles + tile).
//  k_dcrop:   copies each window out of the staging surface to the caller's rows (any pitch).
#include "hoh_dec.h"
#include "hoh_rowmove.h"

// Both kernels are bound by memory latency / bandwidth and tiny beside the decode: no LDS, no
// barriers, one wave per unit of work.

__global__ __launch_bounds__(64) void k_dregion(RegionArgs a, const DecTile* table, DecTile* tiles, uint32_t* gid,
                                                uint32_t* gerr) {
  const int f = blockIdx.x, lane = threadIdx.x;
  // the first tile of this file in the job: the cover sizes of the files before it
  int base = 0;
  for (int i = lane; i < f; i += 64) {
    int tx0, ty0, ntx, nty;
    region_cover_hd(a.tw, a.th, a.xy[2 * i], a.xy[2 * i + 1], a.w, a.h, &tx0, &ty0, &ntx, &nty);
    base += ntx * nty;
  }
  for (int o = 32; o; o >>= 1) base += __shfl_xor(base, o);
  int tx0, ty0, ntx, nty;
  region_cover_hd(a.tw, a.th, a.xy[2 * f], a.xy[2 * f + 1], a.w, a.h, &tx0, &ty0, &ntx, &nty);
  // the host sized every buffer from the same covers; a disagreement fails the job instead of
  // writing past them
  if (tx0 < 0 || ty0 < 0 || tx0 + ntx > a.xt || ty0 + nty > a.yt || base + ntx * nty > a.ntiles) {
    if (lane == 0) atomicOr(gerr, 1u);
    return;
  }
  for (int k = lane; k < ntx * nty; k += 64) {
    const int cy = k / ntx, cx = k - cy * ntx;
    const int tx = tx0 + cx, ty = ty0 + cy;
    const uint32_t g = (uint32_t)f * (uint32_t)a.file_tiles + (uint32_t)(ty * a.xt + tx);
    DecTile t;
    t.x0 = cx * a.tw;
    t.y0 = f * a.sh + cy * a.th;
    t.w = min(a.tw, a.W - tx * a.tw);
    t.h = min(a.th, a.H - ty * a.th);
    t.off = table[g].off;
    t.mode = 0; t.nmatch = 0; t.err = 0; t.gen = 0;
    tiles[base + k] = t;
    gid[base + k] = g;
  }
}

// One wave per window row (wave_move_row, hoh_rowmove.h).  Source (staging) and destination agree
// mod 16 for many windows (both pitches multiples of 16, x * 3 too): 16-byte moves between a byte
// head and tail.  Otherwise the destination still gets aligned dword stores, each assembled from
// the two source dwords that hold it.
#define CROP_ROWS 4      // rows (waves) per workgroup
__global__ __launch_bounds__(64 * CROP_ROWS) void k_dcrop(RegionArgs a, const uint8_t* stage, uint8_t* dst, size_t pitch,
                                                          const uint32_t* gerr) {
  if (*(volatile const uint32_t*)gerr) return;               // a failed decode leaves the caller's buffer alone
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const int r = blockIdx.x * CROP_ROWS + (threadIdx.x >> 6);
  if (r >= a.h) return;
  const int x = a.xy[2 * f], y = a.xy[2 * f + 1];
  const int sx = x - (x / a.tw) * a.tw, sy = y - (y / a.th) * a.th;   // the window inside its cover
  const uint8_t* s = stage + (((size_t)f * a.sh + sy + r) * a.sw + sx) * 3;
  uint8_t* d = dst + ((size_t)f * a.h + r) * pitch;
  wave_move_row(s, d, (uint32_t)a.w * 3, lane);
}

void launch_dregion(const RegionArgs& a, const DecTile* table, DecTile* tiles, uint32_t* gid, uint32_t* gerr,
                    hipStream_t s) {
  hipLaunchKernelGGL(k_dregion, dim3(a.n), dim3(64), 0, s, a, table, tiles, gid, gerr);
}

void launch_dcrop(const RegionArgs& a, const uint8_t* stage, uint8_t* dst, size_t pitch, const uint32_t* gerr,
                  hipStream_t s) {
  hipLaunchKernelGGL(k_dcrop, dim3((a.h + CROP_ROWS - 1) / CROP_ROWS, a.n), dim3(64 * CROP_ROWS), 0, s, a, stage, dst, pitch,
                     gerr);
}
