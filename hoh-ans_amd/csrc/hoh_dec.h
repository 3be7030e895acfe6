// Decoder-side internal definitions (k_decode.hip, hoh_decode.cpp).
#pragma once
#include "hoh_internal.h"

struct hoh_index;
struct hoh_ctx;

struct IndexStream {      // one stream of an encoded image, as recorded by the encoder
  uint64_t payload_off;   // byte offset (in the .hoh) of the first rANS payload word
  uint32_t n;             // symbols
  uint32_t mode;          // SM_*
  uint32_t widx_end;      // slab index of the first payload word (checkpoint widx base)
  uint32_t ckpt_off;      // first checkpoint of the stream in the index
  uint32_t words;
  uint32_t pad;
};

struct DecStream {        // one stream of a .hoh, as parsed by the decoder
  uint64_t table_off;     // where the frequency table bits start (byte), for the table kernel
  uint64_t payload_off;   // first payload byte (rANS words or stored bits)
  uint64_t out_off;       // element offset of the decoded symbols in the decode arena
  uint32_t n, range, pb, mode, tsm, maxbits;
  uint32_t words;         // rANS payload words
  uint32_t err;
  int32_t ix;             // matching index stream, -1 if none
  uint32_t blk;           // 1: decoded into the blocked plane layout (blk_pos, k_decode.hip)
};

struct DecTile {
  int32_t x0, y0, w, h;
  uint64_t off;           // byte offset of the tile in the file
  uint32_t mode, nmatch;
  uint32_t err, gen;      // gen: 1 = a general tile (GenTile), decoded by k_dgen
};

// General tiles: anything beyond the -s0 shape (mode 128, three LZ streams, 1x1 0x0010 layers) --
// RGB mode 2, a fourth LZ stream (16-bit distances), layers with a predictor map.  Their extra
// streams (the fourth LZ stream and the three map streams) take the stream slots
// [ntiles * SK_PER_TILE + 4 t, + 4), behind the numbering the side index matches on.
#define HOH_GEN_MAPCAP 4096   // predictor-map cells per layer the decoder takes (a 4-px grid on a 256^2 tile)
#define HOH_GEN_XS 4          // extra stream slots per tile: the fourth LZ stream, then the three maps
struct GenLayer {
  uint32_t xt, yt;        // predictor grid
  uint32_t nmask;         // masks listed in the layer header (1..16)
  uint32_t mapped;        // 1: a map stream of xt * yt indices into masks; 0: masks[0] everywhere
  uint16_t masks[16];
};
struct GenTile {
  uint32_t nlz;           // LZ streams (3 or 4)
  uint32_t pad;
  GenLayer L[3];
};

#define HOH_DEC_NBUF 20      // slots 16..18: a region decode's staging surface, whole-file tile table and gid;
                             //   19: a mixed batch's tile table (MixedTab)
                             //   (16 is a mixed-shape batch's staging surface too)
struct DecWork {
  void* bufs[HOH_DEC_NBUF] = {nullptr};
  size_t sizes[HOH_DEC_NBUF] = {0};
  hipEvent_t noix_ev = nullptr;   // recorded after this context's last no-index chain kernel
  int noix_dev = -1;              // device it is registered on (k_decode.hip, noix_busy)
  int64_t noix_t = 0;             // host time (steady clock, us) of its last no-index decode
};

// Region decode (hoh_decode_region*, k_region.hip): the w x h window at (xy[2i], xy[2i+1]) of file
// i of n files of one W x H shape.  Passed to k_dregion / k_dcrop by value (the windows are host
// data of the call; 256 pairs are 2 KB of kernel arguments), so no host buffer outlives the call.
#define HOH_REGION_MAX_BATCH 256
struct RegionArgs {
  int32_t n;                        // files
  int32_t W, H, xt, yt, tw, th;     // the files' geometry (hoh_tiling)
  int32_t w, h;                     // the window's size
  int32_t file_tiles;               // xt * yt
  int32_t sw, sh;                   // staging slab of one file: pitch in pixels (a multiple of 16), rows
  int32_t ntiles;                   // covered tiles of all files (the job's tile count)
  int32_t xy[2 * HOH_REGION_MAX_BATCH];
};
// tile rectangle covering pixels [x, x+w) x [y, y+h): tile columns / rows start at multiples of
// tw / th (the last ones may be narrower), so the cover is a pair of divisions
__host__ __device__ inline void region_cover_hd(int tw, int th, int x, int y, int w, int h, int* tx0, int* ty0,
                                                int* ntx, int* nty) {
  *tx0 = x / tw; *ty0 = y / th;
  *ntx = (x + w - 1) / tw - *tx0 + 1;
  *nty = (y + h - 1) / th - *ty0 + 1;
}
void launch_dregion(const RegionArgs& a, const DecTile* table, DecTile* tiles, uint32_t* gid, uint32_t* gerr,
                    hipStream_t s);
void launch_dcrop(const RegionArgs& a, const uint8_t* stage, uint8_t* dst, size_t pitch, const uint32_t* gerr,
                  hipStream_t s);
struct RegionJob {                  // what decode_run needs beside the DecJob of a region decode
  RegionArgs a;
  uint8_t* dst;                     // the caller's buffer and pitch (bytes)
  size_t pitch;
};

// Mixed-shape batch decode (hoh_decode_mixed_async, k_mixed.hip): what decode_run needs beside the
// DecJob.  k_dmixed is the job's front (header check + one DecTile per file, instead of k_dhdr and
// k_dtable), k_mscatter its back (staging surface -> the caller's packed images).
struct MixedJob {
  MixedDims d;
  uint8_t* dst;                     // the caller's packed images
  // a batch with tiled images: files of different tile counts on a vertically packed surface
  // (k_mtab's tile table; k_dtable_mtab is the front, k_dparse_file the parse)
  int tiled;
  int rows;                         //   surface rows: the sum of the heights
};
void launch_dmixed(const MixedDims& d, const uint8_t* in, uint64_t size, uint64_t stride, DecTile* tiles,
                   uint32_t* gerr, hipStream_t s);

void dec_free(DecWork& w);
void noix_release(DecWork& w);
int index_capture(hoh_index* idx, const EncodeJob& j, hipStream_t s);
int index_reserve(hoh_index* idx, size_t nstreams, size_t nck);
Checkpoint* index_ckpt_buf(hoh_index* idx);
void launch_index_capture(const EncodeJob& j, IndexStream* is, size_t per, hipStream_t s);
const IndexStream* index_streams(const hoh_index* idx);
const Checkpoint* index_ckpts(const hoh_index* idx);
int index_nstreams(const hoh_index* idx);
void index_clear(hoh_index* idx);                          // the empty index: no streams, nimg 1, stride 0
IndexStream* index_stream_buf(hoh_index* idx);
// a built index (k_decode.hip, index_build_impl): nstreams records and nck checkpoints are in
// place on the device, in the compact layout; copies the records to the host
int index_commit(hoh_index* idx, int nstreams, size_t nck, hipStream_t s);
void launch_index_pack(const IndexStream* is, const Checkpoint* ck, const uint32_t* dst_off, int nstreams, void* dst,
                       int rec12, hipStream_t s);
int index_build_impl(hoh_ctx* c, const uint8_t* d_in, size_t size, hoh_index* idx, int* Wp, int* Hp, hipStream_t s);
int index_batch(const hoh_index* idx, uint64_t* stride);    // images and file stride the index was recorded for
DecWork& ctx_dec(hoh_ctx* c);
hipStream_t ctx_stream(hoh_ctx* c, void* s);
uint64_t* ctx_pinned(hoh_ctx* c);
int ctx_device(hoh_ctx* c);
int ctx_cus(hoh_ctx* c);
int ctx_noix(hoh_ctx* c);                  // HOH_OPT_NOIX_DECODER (include/hoh_ans.h)
int ctx_decodable(hoh_ctx* c);             // HOH_OPT_DECODABLE
int ctx_small(hoh_ctx* c);                 // HOH_OPT_SMALL_IMAGES
void ctx_mark(hoh_ctx* c, hipStream_t s, const char* name, bool reset);

// Per-context device scratch for the host-buffer entry points (encode_entropy, decode_entropy,
// layer_*, the predictor/unpredictor drop-ins): a grow-only chunk list used as a stack.  A frame
// releases everything allocated after it was opened; after the first call of a given shape no
// call allocates device memory.  alloc() returns nullptr on failure.
struct ScratchFrame {
  hoh_ctx* c;
  size_t cur, used;
  explicit ScratchFrame(hoh_ctx* ctx);
  ~ScratchFrame();
  void* alloc(size_t n);
  template <class T> T* get(size_t n) { return (T*)alloc(n); }
};
