// Mixed-shape batches (hoh_encode_mixed_async / hoh_decode_mixed_async): the front and the back of
// a job whose tiles have many shapes.  First the all-small form, n small-class images as n tiles.  The encoder (k_front.hip .. k_assemble.hip)
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
// A batch that holds tiled images (any side of 512 or more) has files of different tile counts
// and takes the _tab forms: the surface is packed vertically (image i on rows [Y_i, Y_i + H_i) of
// one pitch, no slabs of hmax rows), and a table on the device names every job tile's image,
// rectangle and number inside its file (MixedTab, hoh_internal.h).
//  k_mtab_files / k_mtab_tiles: that table, from the dims passed by value.
//  k_mgather_tab / k_mscatter_tab: one wave per surface row, its image found through Y_i.
//  k_mheader_tab: header, and a tiled image's two tiling bytes.
// (the decoder's front of such a batch is k_dtable_mtab, beside k_dtable in k_decode.hip)
#include "hoh_dec.h"
#include "hoh_rowmove.h"

// All of these are bound by memory latency / bandwidth and tiny beside the coding: no LDS, no
// barriers, one wave per unit of work.

// byte offset of image f in the packed buffer: a prefix over at most 256 products, by every lane
// of a wave (64 bits: tiled images pass 2^32 together)
__device__ __forceinline__ uint64_t mixed_off(const MixedDims& d, int f, int lane) {
  uint64_t v = 0;
  for (int k = lane; k < f; k += 64) v += 3ull * (uint64_t)d.wh[2 * k] * (uint64_t)d.wh[2 * k + 1];
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

// ---- batches with tiled images: the tile table and the vertically packed surface

// Per file: its first job tile T_i, its first surface row Y_i and its packed byte offset, three
// exclusive prefix sums over up to 256 entries: a scan inside each of the four waves, then the
// waves' totals through LDS.
__global__ __launch_bounds__(HOH_MIXED_MAX_BATCH) void k_mtab_files(MixedDims d, MixedTab tab) {
  __shared__ uint64_t ws[3][HOH_MIXED_MAX_BATCH / 64];
  const int i = threadIdx.x, lane = i & 63, wv = i >> 6;
  uint64_t v[3] = {0, 0, 0};
  if (i < d.n) {
    const int W = d.wh[2 * i], H = d.wh[2 * i + 1];
    int xt, yt, tw, th;
    mixed_tiling(W, H, xt, yt, tw, th);
    v[0] = (uint64_t)xt * yt; v[1] = (uint64_t)H; v[2] = 3ull * (uint64_t)W * (uint64_t)H;
  }
  uint64_t a[3] = {v[0], v[1], v[2]};
#pragma unroll
  for (int q = 0; q < 3; q++) {
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t u = __shfl_up(a[q], o);
      if (lane >= o) a[q] += u;
    }
    if (lane == 63) ws[q][wv] = a[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 3; q++)
    for (int k = 0; k < wv; k++) a[q] += ws[q][k];
  if (i < d.n) {
    tab.first[i] = (int32_t)(a[0] - v[0]);
    tab.y[i] = (int32_t)(a[1] - v[1]);
    tab.off[i] = a[2] - v[2];
    if (i == d.n - 1) { tab.first[d.n] = (int32_t)a[0]; tab.y[d.n] = (int32_t)a[1]; tab.off[d.n] = a[2]; }
  }
}

// the last i in [0, n) with a[i] <= v (a strictly ascending, a[0] = 0 <= v)
__device__ __forceinline__ int mixed_find(const int32_t* a, int n, int v) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// per job tile: its image, its number inside its file and its rectangle on the surface
__global__ __launch_bounds__(256) void k_mtab_tiles(MixedDims d, MixedTab tab) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= tab.ntiles) return;
  const int i = mixed_find(tab.first, d.n, t);
  const int W = d.wh[2 * i], H = d.wh[2 * i + 1];
  int xt, yt, tw, th;
  mixed_tiling(W, H, xt, yt, tw, th);
  MixedTile m;
  m.img = i;
  m.k = t - tab.first[i];
  const int tx = m.k % xt, ty = m.k / xt;
  m.x0 = tx * tw; m.y0 = tab.y[i] + ty * th;
  m.w = min(tw, W - tx * tw); m.h = min(th, H - ty * th);
  tab.tile[t] = m;
  tab.tfile[t] = (uint32_t)i;
}

// One wave per surface row; the row's image through Y_i.  What k_mgather / k_mscatter say about the
// caller's buffer holds here too.
__global__ __launch_bounds__(64 * MIX_ROWS) void k_mgather_tab(MixedTab tab, const uint8_t* packed, uint8_t* stage) {
  const int lane = threadIdx.x & 63;
  const int R = blockIdx.x * MIX_ROWS + (threadIdx.x >> 6);
  if (R >= tab.rows) return;                                  // wave-uniform
  const int f = mixed_find(tab.y, tab.n, R);
  const int r = R - tab.y[f];
  const uint32_t nb = (uint32_t)((tab.off[f + 1] - tab.off[f]) / (uint64_t)(tab.y[f + 1] - tab.y[f]));   // 3 * w
  const uint8_t* s = packed + tab.off[f] + (size_t)r * nb;
  uint8_t* o = stage + (size_t)R * tab.pitch * 3;
  wave_move_row(s, o, nb, lane);
}

__global__ __launch_bounds__(64 * MIX_ROWS) void k_mscatter_tab(MixedTab tab, const uint8_t* stage, uint8_t* packed,
                                                                const uint32_t* gerr) {
  if (*(volatile const uint32_t*)gerr) return;               // a failed decode leaves the caller's buffer alone
  const int lane = threadIdx.x & 63;
  const int R = blockIdx.x * MIX_ROWS + (threadIdx.x >> 6);
  if (R >= tab.rows) return;
  const int f = mixed_find(tab.y, tab.n, R);
  const int r = R - tab.y[f];
  const uint32_t nb = (uint32_t)((tab.off[f + 1] - tab.off[f]) / (uint64_t)(tab.y[f + 1] - tab.y[f]));
  const uint8_t* s = stage + (size_t)R * tab.pitch * 3;
  uint8_t* o = packed + tab.off[f] + (size_t)r * nb;
  wave_move_row(s, o, nb, lane);
}

// header, then a tiled image's tiling bytes; nothing for a file whose stride cannot hold them
__global__ void k_mheader_tab(MixedDims d, uint8_t* out, uint64_t stride) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.n) return;
  uint8_t hb[16];
  const uint32_t hl = mixed_prefix_bytes(d, i, hb);
  if (hl > stride) return;
  uint8_t* o = out + (uint64_t)i * stride;
#pragma unroll
  for (uint32_t k = 0; k < 14; k++)
    if (k < hl) o[k] = hb[k];
}

void launch_mtab(const MixedDims& d, const MixedTab& tab, hipStream_t s) {
  hipLaunchKernelGGL(k_mtab_files, dim3(1), dim3(HOH_MIXED_MAX_BATCH), 0, s, d, tab);
  hipLaunchKernelGGL(k_mtab_tiles, dim3((tab.ntiles + 255) / 256), dim3(256), 0, s, d, tab);
}

void launch_mgather_tab(const MixedTab& tab, const uint8_t* packed, uint8_t* stage, hipStream_t s) {
  hipLaunchKernelGGL(k_mgather_tab, dim3((tab.rows + MIX_ROWS - 1) / MIX_ROWS), dim3(64 * MIX_ROWS), 0, s, tab, packed, stage);
}

void launch_mscatter_tab(const MixedTab& tab, const uint8_t* stage, uint8_t* packed, const uint32_t* gerr, hipStream_t s) {
  hipLaunchKernelGGL(k_mscatter_tab, dim3((tab.rows + MIX_ROWS - 1) / MIX_ROWS), dim3(64 * MIX_ROWS), 0, s, tab, stage,
                     packed, gerr);
}

void launch_mheader_tab(const MixedDims& d, uint8_t* out, uint64_t stride, hipStream_t s) {
  hipLaunchKernelGGL(k_mheader_tab, dim3((d.n + 63) / 64), dim3(64), 0, s, d, out, stride);
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
