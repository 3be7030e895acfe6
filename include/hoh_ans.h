/*
 * hoh_ans.h -- C ABI of libhohgpu.so, the MI355X (gfx950) implementation of the hoh-ANS hot path:
 * subtract-green colour transform, MED predictor / unpredictor, greedy RGB LZ, rans64 entropy
 * stream coding and the .hoh tile container of `choh -s0` / `dhoh`.
 *
 * Conventions: plain pointers and sizes, integer status codes (HOH_OK == 0), no exceptions or
 * C++ types across the boundary.  "d_" pointers are device (HBM) buffers; the others are host
 * buffers.  `stream` is a hipStream_t passed as void* (NULL = the context's own stream).
 * One context per host thread per device; contexts own grow-only device workspaces.
 *
 * Each entry point names the reference interface it replaces (hohMiyazawa/hoh-ANS @ v1,
 * file:line).  The reference has no FFI of its own: its API is the set of free functions in
 * the headers below, compiled into the choh / dhoh drivers.  include/hoh/ headers re-expose those
 * exact C++ signatures on top of this ABI.
 */
#ifndef HOH_ANS_H
#define HOH_ANS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------- */
#define HOH_OK 0
#define HOH_E_ARG 1             /* invalid argument                                            */
#define HOH_E_CAP 2             /* output capacity too small (*written / *out_size = needed)   */
#define HOH_E_HIP 3             /* a HIP runtime call failed                                   */
#define HOH_E_RANGE 4           /* symbol >= range, or range / prob_bits outside the supported
                                   set (normalize_freqs assert, stattools.hpp:14)               */
#define HOH_E_UNREPRODUCIBLE 5  /* the reference writes uninitialised bytes for this input
                                   (grey non-binary tiles, choh.cpp:196-205; palette prefix
                                   longer than the indexed layer, choh.cpp:301-308)             */
#define HOH_E_UNSUPPORTED 6     /* valid but not implemented on this path (4-channel formats);
                                   decoder: grey / bitimage / indexed (mode 127) tiles, which
                                   carry no pixel data or no palette, nested tiling,
                                   compaction layers, predictor maps of more than 4096 cells.
                                   -s>=1 files written WITHOUT HOH_OPT_DECODABLE are parsed like
                                   any other file now: their stale layers (Q14) read as
                                   HOH_E_CORRUPT, or decode to wrong pixels where the stale
                                   stream happens to parse                                      */
#define HOH_E_CORRUPT 7         /* decoder: malformed or undecodable bitstream (incl. the
                                   reference's lossy raw tables)                     */
#define HOH_E_NODEV 8           /* no GPU / HIP device unavailable                              */

typedef struct hoh_ctx hoh_ctx;

int hoh_ctx_create(hoh_ctx** ctx, int device);
void hoh_ctx_destroy(hoh_ctx* ctx);
const char* hoh_strerror(int code);
/* The context's own HIP stream (what a NULL `stream` argument means), as void*: callers that
 * order their own streams against it with events (the Python mirror fences torch's default
 * stream this way). */
void* hoh_ctx_stream(hoh_ctx* ctx);
const char* hoh_version(void);
/* Number of device allocations (hipMalloc) the library has made so far, process-wide.  Contexts
 * keep grow-only workspaces, so repeated calls of one shape allocate nothing after the first. */
uint64_t hoh_device_alloc_count(void);
/* per-kernel device time of the last call, for measurement (ms); enable with hoh_set_profiling */
void hoh_set_profiling(hoh_ctx* ctx, int on);
int hoh_get_kernel_ms(hoh_ctx* ctx, const char** names, float* ms, int max);
/* Per-kernel totals accumulated over every profiled call since the last reset (names are the
 * kernel stages; total_ms / count give the average launch duration on the call's stream). */
int hoh_get_kernel_stats(hoh_ctx* ctx, const char** names, double* total_ms, uint64_t* count, int max);
void hoh_reset_kernel_stats(hoh_ctx* ctx);

/* Per-context options (HOH_E_ARG for an unknown option or value).
 * HOH_OPT_NOIX_DECODER picks the rANS chain kernel of decodes WITHOUT a side index (any foreign
 * .hoh, dhoh.cpp:297-396; every stream one serial chain): HOH_NOIX_ADAPTIVE (default: one lane per
 * chain with full tables while the decode has the device to itself, compact-table lanes beside
 * other no-index decodes), HOH_NOIX_LANES (compact tables, up to 64 chains per workgroup),
 * HOH_NOIX_MULTI (full tables, 12 chains per CU) or HOH_NOIX_WAVE (one wave per stream).  Every
 * choice gives the same bytes; the library reads no environment variables for it.  hoh_index_build
 * walks the same chains and follows the option (lanes or multi; HOH_NOIX_WAVE reads as adaptive). */
#define HOH_OPT_NOIX_DECODER 1
#define HOH_NOIX_ADAPTIVE (-1)
#define HOH_NOIX_LANES 0
#define HOH_NOIX_MULTI 1
#define HOH_NOIX_WAVE 2
/* HOH_OPT_DECODABLE (0 default, 1): every encode entry point of the context, hoh_layer_encode
 * included, writes files that can be read back at any speed.  At 0 the files are the reference's
 * byte for byte, whose -s1..-s4 layers announce a predictor map and then carry a truncated prefix of
 * a stale stream.  At 1:
 *  - a layer is its header, its map stream and ONE whole entropy stream of the residuals the header
 *    describes (at -s>=1 with a grid larger than 1x1 the searched, LZ-cleaned residuals, otherwise
 *    the MED residuals).  With s(pb) the stream's size at prob_bits pb, the candidates are 16, 17,
 *    18, 19 if s(16) < s(15), else 15, 14, 13, 12, and the layer takes the first candidate of
 *    strictly smallest size (the reference ladder's own evaluation set, layer_encode.hpp:326-392);
 *    -s0 layers stay MED at prob_bits 15;
 *  - a tile is sub-green (mode 128) unless, at -s>=3, the three plain planes sum strictly smaller
 *    (RGB, mode 2, choh.cpp:309); the grey, bitimage and indexed modes carry no decodable pixel
 *    data (Q15) and are never taken, so HOH_E_UNREPRODUCIBLE cannot arise;
 *  - the vertical LZ search stops at distance 65535: the reference's 65536 does not fit the two
 *    distance bytes and reads back as 0 (lz.hpp:55, :85-87);
 *  - no stream (hoh_encode_entropy included) takes the raw frequency table where it would drop a
 *    frequency's high bits (Q4: a predictor map over a few masks always would); it takes the
 *    clamped table instead.
 * Not covered: hoh_mgpu_* (its contexts are its own) and header-only (untiled, Q13) files; with
 * HOH_OPT_SMALL_IMAGES the small class of untiled images gets a real file, and this option then
 * applies to its one tile as to any other. */
#define HOH_OPT_DECODABLE 2
/* HOH_OPT_CHAIN_TABLES: where the prob_bits-15 encoder chains (every -s0 plane, hoh_encode_entropy
 * at prob_bits 15) read their symbol tables from.  HOH_CHAIN_TABLES_LDS keeps each stream's 32 most
 * probable consecutive symbols in LDS and gathers only the others from memory;
 * HOH_CHAIN_TABLES_GLOBAL gathers every entry from memory; HOH_CHAIN_TABLES_AUTO (default) chooses
 * per launch.  Every choice gives the same bytes and the same side index. */
#define HOH_OPT_CHAIN_TABLES 3
#define HOH_CHAIN_TABLES_AUTO 0
#define HOH_CHAIN_TABLES_LDS 1
#define HOH_CHAIN_TABLES_GLOBAL 2
/* HOH_OPT_SMALL_IMAGES (0 default, 1): images of the SMALL CLASS, W <= 511 and H <= 511 (all of
 * them untiled, choh.cpp:454-461), are written and read as single-tile files.  At 0 the library
 * follows the reference: choh codes the one tile, discards it and writes the 8-10 byte header
 * (SURVEY Q13), and every decode, enqueue-only, batched and index entry point answers
 * HOH_E_UNSUPPORTED for an untiled shape.  At 1:
 *  - hoh_encode_image / _ix write header || tile, the tile coded straight into d_out behind the
 *    header: exactly the bytes the reference's dhoh reads (dhoh.cpp:379 calls decode_tile right after
 *    the header) and choh throws away, so *out_size == *printed.  The tile is what the context's
 *    other options make it: without HOH_OPT_DECODABLE the reference's bytes at every speed (palette
 *    tiles, mode 127, and HOH_E_UNREPRODUCIBLE for non-binary grey included); with it a decodable
 *    sub-green or RGB tile.  At -s0 _ix records the side index (7 streams);
 *  - hoh_decode_image / _ix read such a file (header, the tile's own tiling bytes 0 0, one tile of
 *    W x H) with or without an index.  A file that ends with the header (choh's header-only file)
 *    stays HOH_E_UNSUPPORTED, nested tiling (nonzero tiling bytes) is HOH_E_UNSUPPORTED, truncation
 *    or junk HOH_E_CORRUPT;
 *  - hoh_encode_image_async, hoh_decode_image_async, hoh_encode_images_async and
 *    hoh_decode_images_async accept the shape.  A batch of n is ONE job for any H: the n images are
 *    the n tiles of their W x n*H stack; file i lies at i * stride, byte-identical to the
 *    synchronous call's; one side index serves the batch and equals hoh_index_concat of the n
 *    single indexes.  -s>=1 batches run in stacks bounded by their pixels;
 *  - hoh_index_build accepts a small-class file of the -s0 shape.
 * Untiled shapes OUTSIDE the small class (one side under 256, the other 512 or more) behave as at
 * 0 on every entry point: the decoder's LDS rows and rings are sized for tiles under 512 wide.
 * Not covered either way: hoh_decode_region* and hoh_region_cover (HOH_E_UNSUPPORTED for untiled
 * shapes), hoh_encode_tiles* / hoh_decode_tiles*, hoh_mgpu_*.  Batches of mixed shapes have calls of
 * their own, hoh_encode_mixed_async / hoh_decode_mixed_async, which need no option. */
#define HOH_OPT_SMALL_IMAGES 4
int hoh_ctx_set_option(hoh_ctx* ctx, int option, int64_t value);

/* ---- image level: `choh in out W H -sN` / `dhoh in out` -------------------------------- */

/* Worst-case .hoh size for a W x H image (stored planes + LZ streams + framing). */
size_t hoh_encode_bound(int W, int H);

/* Replaces choh.cpp:394-527.  speed = cruncher_mode (-s0 .. -s4; choh.cpp:408-427).  Reads
 * W*H*3 interleaved RGB bytes from d_rgb, writes the exact bytes choh writes (header-only for
 * untiled images; header || tile for the small class under HOH_OPT_SMALL_IMAGES) to
 * d_out.  *out_size = bytes written; *printed (optional) = the number choh prints (choh.cpp:522).  -s1..-s4 run the predictor search, seek-distance LZ and
 * prob_bits ladder (layer_encode.hpp:122-392) and get no side index.  Without HOH_OPT_DECODABLE
 * their files are the reference's, undecodable by construction; with it they read
 * back through every decode entry point. */
int hoh_encode_image(hoh_ctx* ctx, const uint8_t* d_rgb, int W, int H, int speed,
                     uint8_t* d_out, size_t cap, size_t* out_size, size_t* printed, void* stream);

/* Decode side index: the encoder's coder state every 256 symbols of each plane stream (a
 * Recoil-style checkpoint list kept BESIDE the .hoh, never inside it -- the file bytes are
 * identical with or without it).  With an index the decoder splits every stream into
 * independent segments; without one (any foreign .hoh) it decodes each stream serially.  A
 * segment whose end state disagrees with the next checkpoint fails the decode (HOH_E_CORRUPT). */
typedef struct hoh_index hoh_index;
int hoh_index_create(hoh_index** idx);
void hoh_index_destroy(hoh_index* idx);
size_t hoh_index_bytes(const hoh_index* idx);
int hoh_encode_image_ix(hoh_ctx* ctx, const uint8_t* d_rgb, int W, int H, int speed,
                        uint8_t* d_out, size_t cap, size_t* out_size, size_t* printed,
                        hoh_index* idx, void* stream);
/* An EMPTY index (no streams: a fresh one, the one a -s1..-s4 encode leaves, a failed build or
 * load) is accepted by every decode entry point as no index at all, whatever n and stride. */

/* ---- side index beside the file: save, load, build, concatenate -------------------------
 * hoh_index_serialize writes the index as a little-endian, position-independent blob (a sidecar
 * file next to the .hoh); hoh_index_deserialize reads it back on any context or process.  The
 * blob is canonical: indexes that describe the same streams of the same bytes serialize to the
 * same bytes, whether an encode recorded them, hoh_index_build made them from the file or
 * hoh_index_concat joined them.
 *   header, 48 B:        'H','O','H','X'; u32 version = 1; u32 seg = 256 (symbols per checkpoint);
 *                        u32 nstreams; u32 nimg; u32 0; u64 stride (0 when nimg == 1); u64 nck; u64 0
 *   nstreams x 24 B:     u64 payload_off; u32 n; u32 mode; u32 words; u32 0
 *   nck x 12 B:          u32 xl; u32 xh; u32 wi
 * Stream s = tile * 7 + kind (kinds: three LZ streams, G, R, B planes, the indexed plane), tiles
 * of a batch in image order.  mode: 0 empty or not in the file (the indexed plane of a sub-green
 * tile, the planes of a palette tile), 1 rANS, 2 stored; a record whose mode is not 1 is zero
 * elsewhere.  payload_off = byte of the first rANS payload word in the .hoh (in the batch buffer
 * when nimg > 1: file i starts at i * stride); n = symbols; words = payload words.  A rANS stream
 * owns ceil(n / seg) checkpoints, stored in stream order (its first one is the running sum of the
 * streams before it; nck is the total): checkpoint k = the coder state (xh << 32 | xl) before
 * symbol k * seg and wi = the index, inside the stream's own payload, of the next word the decoder
 * reads.  The blob's length is exactly 48 + 24 nstreams + 12 nck; an empty index is its header.
 * `stream` orders the calls behind the work that recorded the index (an encode enqueued on it);
 * NULL waits for the whole device instead.  All three calls return with their work finished. */
size_t hoh_index_serialized_size(const hoh_index* idx);    /* 0 on failure; waits for the device
                                                              when an encode recorded idx         */
/* HOH_E_CAP (with *written = the size needed) when cap is too small. */
int hoh_index_serialize(const hoh_index* idx, uint8_t* out, size_t cap, size_t* written, void* stream);
/* The blob is untrusted: it is validated on the host before any device call -- magic, version,
 * seg, the reserved fields, nstreams a multiple of 7 and of nimg >= 1, stride == 0 exactly when
 * nimg == 1, modes, zero non-rANS records, sum of ceil(n / seg) == nck, exact length (computed
 * without overflow).  Any violation: HOH_E_CORRUPT and idx empty.  A well-formed blob with wrong
 * VALUES (of another file, or edited) is safe to decode with: a stream's record is used only when
 * its payload_off, n and words equal what the decoder parsed from the file, every payload read is
 * bounded by the file size, and a wrong state fails the decode (HOH_E_CORRUPT) or, where no
 * checkpoint matches, leaves the stream to the serial decoder. */
int hoh_index_deserialize(hoh_index* idx, const uint8_t* blob, size_t size, void* stream);
/* An index for any .hoh, from its bytes alone (d_hoh: `size` bytes on the device; synchronous;
 * W, H optional outputs): the decoder's header / tile / stream parse, then one pass over every
 * rANS chain that stores no symbols, only the checkpoints.  The result serializes to the bytes of
 * the index hoh_encode_image_ix records for the same file.  HOH_E_UNSUPPORTED (idx empty) for a
 * file the indexed decoder does not cover in full: general tiles (RGB mode, a fourth LZ stream,
 * predictor maps -- every HOH_OPT_DECODABLE -s>=1 file), palette / grey / bitimage tiles, a stream
 * with range > 512 or prob_bits > 15, untiled files (except the small class under
 * HOH_OPT_SMALL_IMAGES).  HOH_E_CORRUPT (idx empty) for a chain that
 * runs out of payload or does not end in the initial state, and for any framing error. */
int hoh_index_build(hoh_ctx* ctx, const uint8_t* d_hoh, size_t size, hoh_index* idx, int* W, int* H, void* stream);
/* dst = the index of n files laid out at i * stride, as hoh_decode_images_async reads them, from
 * their n single-image indexes (equal stream counts, else HOH_E_ARG; dst must not be a source).
 * Serializes to the bytes of the index hoh_encode_images_async(n, .., stride, idx) records for the
 * same files.  n == 1 copies (stride ignored). */
int hoh_index_concat(hoh_index* dst, int n, const hoh_index* const* src, uint64_t stride, void* stream);
/* A batch whose files carry DIFFERENT tile counts (hoh_encode_mixed_async with tiled images among
 * its shapes) has an index the version-1 blob cannot hold (one stream count for all files):
 * hoh_index_serialize answers HOH_E_UNSUPPORTED for it and hoh_index_serialized_size 0.  Such an
 * index is persisted file by file:
 * hoh_index_file: dst = file i's own index out of a batch's (recorded, concatenated or joined):
 * payload offsets rebased by i * stride, nimg = 1.  It serializes to the bytes of the index
 * hoh_encode_image_ix records for image i alone.  HOH_E_ARG for i outside the batch; an empty batch
 * index gives an empty dst for any i >= 0.  dst must not be batch.
 * hoh_index_join: hoh_index_concat for any stream counts that are multiples of 7 (HOH_E_ARG
 * otherwise, and for an empty source beside non-empty ones).  Where the counts are equal dst
 * serializes to hoh_index_concat's bytes.  A decode with dst needs the same n and stride (else
 * HOH_E_ARG), as with any batch index. */
int hoh_index_file(const hoh_index* batch, int i, hoh_index* dst, void* stream);
int hoh_index_join(hoh_index* dst, int n, const hoh_index* const* src, uint64_t stride, void* stream);

/* Replaces dhoh.cpp:297-396 (with the decoder defects of SURVEY Q1, Q9-Q12 fixed).  d_hoh holds
 * `size` bytes of a .hoh file; writes W*H*3 RGB bytes to d_rgb.  Every decode entry point reads,
 * whoever wrote the file: tile modes 128 (sub-green) and 2 (RGB); LZ with three or four streams
 * (distance = backby2 << 8 | backby, up to 65535); layers with a predictor map of any grid (up to
 * 4096 cells), 1 to 16 masks of any value, a map stream and a residual stream, stored or rANS at
 * prob_bits up to 19 (16..19 are read from five bits of the metadata byte: the reference's writer
 * carries them into bit 6, its reader masks that bit off).  A wrong map or residual count, a map
 * index that is not below the mask count, or truncation gives HOH_E_CORRUPT.  An -s>=1 file
 * written without HOH_OPT_DECODABLE carries stale layers (Q14): HOH_E_CORRUPT, or wrong pixels
 * where the stale stream happens to parse. */
int hoh_decode_image(hoh_ctx* ctx, const uint8_t* d_hoh, size_t size, uint8_t* d_rgb, size_t cap,
                     int* W, int* H, void* stream);
int hoh_decode_image_ix(hoh_ctx* ctx, const uint8_t* d_hoh, size_t size, uint8_t* d_rgb, size_t cap,
                        int* W, int* H, const hoh_index* idx, void* stream);

/* ---- enqueue-only image path (no host synchronisation) ----------------------------------
 * The work of hoh_encode_image_ix / hoh_decode_image_ix for tiled images, enqueued on `stream`
 * with no host round trip, so one host thread keeps many images in flight on many streams (the
 * reference's choh/dhoh loop over files, choh.cpp:464-500 / dhoh.cpp:297-396, without the
 * per-file wait).  Results are written by the stream to d_status (device or pinned host memory,
 * two u64): d_status[0] = HOH_OK or an HOH_E_* code, d_status[1] = the .hoh size (encode) or
 * W*H*3 (decode).  Read it after synchronising the stream.  Calls on one stream run in order, so
 * a context's workspaces, the index and the caller's buffers may be reused by the next call on
 * the same stream.  The decoder takes W and H from the caller (the file header is checked on the
 * device: a mismatch gives HOH_E_CORRUPT) and reads at most `size` bytes (a bound suffices, e.g.
 * the encoder's cap).  Header-only (untiled) images return HOH_E_UNSUPPORTED here:
 * use the synchronous calls -- unless HOH_OPT_SMALL_IMAGES is set and the shape is of the small
 * class, which these calls then take like a tiled one (a decode whose `size` is exactly the header's
 * length, choh's header-only file, still returns HOH_E_UNSUPPORTED). */
int hoh_encode_image_async(hoh_ctx* ctx, const uint8_t* d_rgb, int W, int H, int speed, uint8_t* d_out,
                           size_t cap, hoh_index* idx, uint64_t* d_status, void* stream);
int hoh_decode_image_async(hoh_ctx* ctx, const uint8_t* d_hoh, size_t size, int W, int H, uint8_t* d_rgb,
                           size_t cap, const hoh_index* idx, uint64_t* d_status, void* stream);

/* ---- batched enqueue-only image path ------------------------------------------------------
 * n images of one shape per call: each kernel of the image path covers the tiles of all n images
 * in one launch (choh.cpp:464-500's tile loop, run over the batch), so a few streams -- and the
 * few hardware queues HIP gives a process by default -- keep the device busy.  Images are
 * contiguous (image i at d_rgb + i*W*H*3); file i is written at / read from d_hoh + i*stride
 * (stride >= each file's size, e.g. hoh_encode_bound(W, H)).  d_status holds 2n u64, {status,
 * size} per image as in the single-image calls: an image's own failures (HOH_E_CAP past its
 * stride, HOH_E_UNREPRODUCIBLE, ...) mark only its slot; a failure of the job marks every slot.
 * Files are byte-identical to the single-image calls'.  One side index serves the whole batch
 * (payload positions are absolute in the batch buffer), so a decode with it needs the same n and
 * stride (else HOH_E_ARG; an empty index passes with any).  The batch runs as one job when its tiles stack -- H a multiple of 256,
 * so the n images are the 256-row tile grid of one n*H image; at -s1..-s4 (whose workspace is ~8 MB
 * per tile) as stacks of up to 1024 tiles (one 8192^2 image, or 64 of 1024^2) one after another,
 * and no side index (idx, if given, is emptied as in the single-image calls); otherwise tiled
 * images run one after another on the stream (without a side index when n > 1 at -s0:
 * HOH_E_UNSUPPORTED).  Untiled shapes (header-only files) return HOH_E_UNSUPPORTED for
 * any n, as in the single-image async calls: use hoh_encode_image / hoh_decode_image -- unless
 * HOH_OPT_SMALL_IMAGES is set and the shape is of the small class: then the batch is one job for
 * any H (the n images are the n single tiles of their W x n*H stack), with one side index.  The decoder
 * bounds every parse of file i by [i*stride, (i+1)*stride) (a truncated file reads as corrupt) and
 * reads n*stride bytes of d_hoh at most; in a one-job batch an error in any file marks every
 * image's status. */
int hoh_encode_images_async(hoh_ctx* ctx, int n, const uint8_t* d_rgb, int W, int H, int speed, uint8_t* d_out,
                            size_t stride, hoh_index* idx, uint64_t* d_status, void* stream);
int hoh_decode_images_async(hoh_ctx* ctx, int n, const uint8_t* d_hoh, size_t stride, int W, int H, uint8_t* d_rgb,
                            const hoh_index* idx, uint64_t* d_status, void* stream);

/* ---- mixed-shape batches: tiled images and small ones in one job ------------------------------
 * n images, each with its own shape, per call: a folder of photos, thumbnails, crops or dataset
 * samples without one call per image and without padding.  Shapes: every shape hoh_tiling tiles
 * ((W >= 512 || H >= 512) && W >= 256 && H >= 256), the small class (W <= 511 and H <= 511, see
 * HOH_OPT_SMALL_IMAGES), and any mix of both in any order; the remaining untiled shapes (one side
 * under 256, the other 512 or more, e.g. 512 x 10) are HOH_E_UNSUPPORTED.  h_wh (host) holds W_0,
 * H_0, W_1, H_1, ... and is read only during the call.  The images are packed back to back on both
 * sides: image i is W_i*H_i*3 bytes at d_rgb + offsets[i] (hoh_mixed_rgb_bytes; 64-bit: tiled
 * images pass 2^32 bytes together).  File i is written at / read from d_hoh + i*stride as in
 * hoh_*_images_async; d_status holds 2n u64, {status, size} per image (decode: size = W_i*H_i*3).
 * Both calls are enqueue-only and need no context option.  File i is what the synchronous call
 * writes for image i alone, byte for byte, at the same speed and options: a tiled image gives
 * hoh_encode_image's file (header, the two tiling bytes, the tile size table, the tiles), a small
 * image header || tile (hoh_encode_image under HOH_OPT_SMALL_IMAGES).  HOH_OPT_DECODABLE,
 * HOH_OPT_NOIX_DECODER and HOH_OPT_CHAIN_TABLES apply as everywhere else.
 * Encode: at -s0 the whole batch is ONE job over the tiles of all its files.  The images pass through
 * a staging surface in the context's workspace: all of the small class, a stack of Wmax x Hmax slabs;
 * with tiled images among them, one surface of pitch Wmax packed vertically, image i on rows
 * [Y_i, Y_i + H_i), Y_i the sum of the heights before it, and a tile table built on the device (one
 * very wide image beside many narrow ones still wastes surface).  idx, if given, records the batch's
 * side index: nimg = n, the batch's stride.  Where all files have the same tile count it serialises
 * to the bytes of hoh_index_concat over the n single-image indexes (for a uniform tiled batch: the
 * blob hoh_encode_images_async records); where they differ, see hoh_index_file / hoh_index_join.
 * At -s1..-s4 maximal runs of consecutive equal shapes run as uniform batches one after another (a
 * run of a tiled shape as hoh_encode_images_async does it, a run of one as a single image), and idx
 * is emptied as in the other -s>=1 calls; between two runs the host waits for the stream, because
 * the search's log2 tables are per pixel count (at most four per job; one tiled shape uses up to
 * four by itself) and the host rebuilds them.  An image's own failure (HOH_E_CAP past its stride,
 * with the size it would need in the size word; HOH_E_UNREPRODUCIBLE) marks only its slot.
 * Decode: one job for every file kind the full decoder reads (decodable -s>=1 general tiles and RGB
 * mode included), with the index, without it, and under every HOH_OPT_NOIX_DECODER choice.  The
 * caller gives every W and H; each file's header and each tiled file's tiling bytes are checked on
 * the device against (W_i, H_i) (a mismatch, or a size table that runs past the file's stride slot:
 * HOH_E_CORRUPT) and every parse of file i stays inside [i*stride, (i+1)*stride).  An error in any
 * file marks every slot and leaves the caller's d_rgb untouched.
 * Returned at once: HOH_E_ARG for n outside 1..HOH_MIXED_MAX_BATCH, null pointers, a non-positive
 * dimension, a sum of heights above 2^30 or more than 2^24 tiles, or a non-empty index recorded for
 * another n or stride; HOH_E_UNSUPPORTED for a shape neither tiled nor of the small class, and for
 * a -s0 job past the encoder's 32-bit table bound (~74,000 tiles); HOH_E_CAP (encode) for a stride
 * under 10 bytes, the longest header of the small class.
 * Workspaces are grow-only: a repeat call with the same shapes allocates nothing, in whatever
 * order they come.
 * Not covered: mixed -s>=1 batches as one job, direct reads and writes of the packed rows (the
 * images pass through the staging surface), hoh_mgpu_*. */
#define HOH_MIXED_MAX_BATCH 256
/* host only: offsets[i] = sum over k < i of 3*W_k*H_k (n+1 entries, may be NULL); returns offsets[n];
 * 0 (offsets untouched) if any shape is neither tiled nor of the small class or n is out of range */
size_t hoh_mixed_rgb_bytes(int n, const int32_t* h_wh, uint64_t* offsets);
int hoh_encode_mixed_async(hoh_ctx* ctx, int n, const uint8_t* d_rgb, const int32_t* h_wh, int speed,
                           uint8_t* d_out, size_t stride, hoh_index* idx, uint64_t* d_status, void* stream);
int hoh_decode_mixed_async(hoh_ctx* ctx, int n, const uint8_t* d_hoh, size_t stride, const int32_t* h_wh,
                           uint8_t* d_rgb, const hoh_index* idx, uint64_t* d_status, void* stream);

/* ---- region decode: a crop of a .hoh by decoding only its tiles ----------------------------
 * The tiles of a .hoh share no state, so a pixel window needs only the tiles it touches.  The
 * calls below restore the w x h window at (x, y): h rows of w*3 RGB bytes, row r at
 * d_rgb + r*pitch (pitch in bytes, >= w*3, any value -- no multiple of 3 or 4 is asked; cap >=
 * (h-1)*pitch + w*3).  No other byte of the caller's buffer is written, and the bytes written
 * equal the same window of what hoh_decode_image restores.  Only the tiles of hoh_region_cover are
 * parsed, entropy-decoded and unpredicted; the tile table is read whole (offsets are prefix sums)
 * and the bytes of other tiles are never read, so a defect in a tile outside the cover does not
 * fail the call, while one inside it fails as in a full decode (HOH_E_CORRUPT /
 * HOH_E_UNSUPPORTED).  Every file kind the full decoder reads is read here, with or without a side
 * index and under every HOH_OPT_NOIX_DECODER choice.  idx is the index of the WHOLE file (batch:
 * of the whole batch, same n and stride, else HOH_E_ARG) however it came to be -- recorded, built,
 * loaded, concatenated; the covered tiles' streams use their checkpoints; an empty index is no
 * index.  HOH_E_ARG: an empty rectangle, one not inside the image, pitch < w*3, n out of range;
 * HOH_E_UNSUPPORTED: an untiled shape (header-only files); HOH_E_CAP: cap too small.
 * The tiles are decoded into a staging surface in the context's workspace (sized for the largest
 * cover a w x h window can have, so after the first call of a shape a repeat call allocates no
 * device memory wherever its window lies) and the window is copied out from there. */
#define HOH_REGION_MAX_BATCH 256
/* host only: the tile rectangle that covers pixels [x, x+w) x [y, y+h) of a W x H image
 * (tiling of hoh_tiling): first tile column / row and the counts.  HOH_E_ARG for an empty
 * rectangle or one not inside the image, HOH_E_UNSUPPORTED for an untiled shape. */
int hoh_region_cover(int W, int H, int x, int y, int w, int h, int* tx0, int* ty0, int* ntx, int* nty);
/* synchronous; reads W, H from the file as hoh_decode_image does (optional outputs) */
int hoh_decode_region(hoh_ctx* ctx, const uint8_t* d_hoh, size_t size, int x, int y, int w, int h,
                      uint8_t* d_rgb, size_t pitch, size_t cap, int* W, int* H,
                      const hoh_index* idx, void* stream);
/* enqueue-only (no host synchronisation); the caller gives W, H, the header is checked on the
 * device (a mismatch: HOH_E_CORRUPT in the status); d_status = {status, w*h*3} */
int hoh_decode_region_async(hoh_ctx* ctx, const uint8_t* d_hoh, size_t size, int W, int H,
                            int x, int y, int w, int h, uint8_t* d_rgb, size_t pitch, size_t cap,
                            const hoh_index* idx, uint64_t* d_status, void* stream);
/* enqueue-only batch, one job: crop i = the w x h window at (h_xy[2i], h_xy[2i+1]) of file i (n
 * files of one shape at d_hoh + i*stride, as hoh_decode_images_async reads them; any tiled shape,
 * stacking or not), written at d_rgb + i*h*pitch; d_status holds 2n u64.  h_xy (host) is read
 * only during the call.  Every parse of file i stays inside [i*stride, (i+1)*stride); an error in
 * any file marks every slot.  n <= HOH_REGION_MAX_BATCH. */
int hoh_decode_regions_async(hoh_ctx* ctx, int n, const uint8_t* d_hoh, size_t stride, int W, int H,
                             const int32_t* h_xy, int w, int h, uint8_t* d_rgb, size_t pitch,
                             const hoh_index* idx, uint64_t* d_status, void* stream);

/* Host-side header parse: W, H and tiling of a .hoh (dhoh.cpp:320-366). */
int hoh_peek_header(const uint8_t* hoh, size_t size, int* W, int* H, int* x_tiles, int* y_tiles);

/* ---- sharded image encode (multi-GPU: one process per GPU) ------------------------------ */

/* Encodes tiles [t0, t0+ntiles) (row-major tile index, choh.cpp:464-500) of the W x H image into
 * a blob of concatenated tile byte strings at d_out; d_tile_sizes (device, ntiles u32) receives
 * each tile's size.  A rank's blob plus everyone's sizes are what the gather exchanges.
 * d_rgb is the base of the whole image: a rank holding only rows [y0, y1) passes
 * (its buffer - y0*W*3); only the pixels of the named tiles are read. */
int hoh_encode_tiles(hoh_ctx* ctx, const uint8_t* d_rgb, int W, int H, int t0, int ntiles,
                     uint8_t* d_out, size_t cap, uint32_t* d_tile_sizes, size_t* out_size,
                     void* stream);
int hoh_encode_tiles_ix(hoh_ctx* ctx, const uint8_t* d_rgb, int W, int H, int t0, int ntiles,
                        uint8_t* d_out, size_t cap, uint32_t* d_tile_sizes, size_t* out_size,
                        hoh_index* idx, void* stream);
/* The same at any speed (-s0..-s4; -s>=1 tiles get no side index). */
int hoh_encode_tiles_speed(hoh_ctx* ctx, const uint8_t* d_rgb, int W, int H, int speed, int t0, int ntiles,
                           uint8_t* d_out, size_t cap, uint32_t* d_tile_sizes, size_t* out_size,
                           hoh_index* idx, void* stream);
/* Decodes tiles [t0, t0+ntiles) from d_blob (their byte strings concatenated, sizes in
 * h_tile_sizes) into the W x H image at d_rgb (only those tiles' pixels are written; d_rgb is
 * the base of the whole image).  idx may be the index hoh_encode_tiles_ix recorded. */
int hoh_decode_tiles(hoh_ctx* ctx, const uint8_t* d_blob, size_t size, int W, int H, int t0, int ntiles,
                     const uint32_t* h_tile_sizes, uint8_t* d_rgb, const hoh_index* idx, void* stream);
/* Enqueue-only forms of the two calls above (no host round trip; see the image-level async
 * calls for the d_status convention).  Encode: d_status[1] = the blob size.  Decode: the tile
 * sizes are read from DEVICE memory (d_tile_sizes, e.g. as the encoder wrote them), so a shard can
 * be decoded before its sizes ever reach the host; d_status[1] = the shard's RGB bytes. */
int hoh_encode_tiles_async(hoh_ctx* ctx, const uint8_t* d_rgb, int W, int H, int speed, int t0, int ntiles,
                           uint8_t* d_out, size_t cap, uint32_t* d_tile_sizes, hoh_index* idx, uint64_t* d_status,
                           void* stream);
int hoh_decode_tiles_async(hoh_ctx* ctx, const uint8_t* d_blob, size_t size, int W, int H, int t0, int ntiles,
                           const uint32_t* d_tile_sizes, uint8_t* d_rgb, const hoh_index* idx, uint64_t* d_status,
                           void* stream);
/* Batched shards (multi-GPU with several images in flight per GPU): the same tile band
 * [t0, t0+ntiles) of n W x H images per call.  The band must be whole tile rows (t0 and ntiles
 * multiples of x_tiles, else HOH_E_ARG).  d_rgb holds the n bands back to back (band i = rows
 * [y0, y1) of image i at d_rgb + i*W*(y1-y0)*3 -- NOT the image base as in the single-shard
 * calls); blob i is written at / read from d_blob + i*stride, its tile sizes at
 * d_tile_sizes + i*ntiles (device u32); d_status holds {status, blob size} (encode) or {status,
 * band RGB bytes} (decode) per shard.  When H is a multiple of 256 the n bands stack into one
 * tile grid and every kernel covers all n shards per launch (as hoh_encode_images_async does for
 * whole images); otherwise the shards run one after another on the stream.  Blobs are
 * byte-identical to n single-shard calls'.  -s1..-s4 stack up to 1024 tiles per job.  A side
 * index serves the batch it was recorded for (same n and stride).  The decoder bounds every parse
 * of blob i by [i*stride, (i+1)*stride) and reads n*stride bytes of d_blob at most; in a one-job
 * batch an error in any blob marks every shard's status. */
int hoh_encode_tiles_images_async(hoh_ctx* ctx, int n, const uint8_t* d_rgb, int W, int H, int speed, int t0,
                                  int ntiles, uint8_t* d_blob, size_t stride, uint32_t* d_tile_sizes, hoh_index* idx,
                                  uint64_t* d_status, void* stream);
int hoh_decode_tiles_images_async(hoh_ctx* ctx, int n, const uint8_t* d_blob, size_t stride, int W, int H, int t0,
                                  int ntiles, const uint32_t* d_tile_sizes, uint8_t* d_rgb, const hoh_index* idx,
                                  uint64_t* d_status, void* stream);
/* Host: the .hoh prefix for a tiled image given every tile's size (choh.cpp:437-498):
 * magic, format, depth, varint W-1, H-1, x_tiles-1, y_tiles-1, n-1 varint sizes.  Returns the
 * prefix length, or 0 if cap is too small. */
size_t hoh_file_prefix(int W, int H, const uint32_t* tile_sizes, int ntiles, uint8_t* out, size_t cap);
/* tiling of choh.cpp:454-461: returns 1 if tiled */
int hoh_tiling(int W, int H, int* x_tiles, int* y_tiles, int* tile_w, int* tile_h);

/* ---- multi-GPU in one process (choh / dhoh over several devices) ----------------------- */

/* One process drives ndev GPUs: a context and a HIP stream per device and, when the devices are
 * distinct, one RCCL communicator each (ncclCommInitAll; librccl.so is loaded here, not at link
 * time).  A device may be listed more than once (several shards on one GPU): the blobs then move
 * by device copies instead of RCCL (hoh_mgpu_transport returns 0; 1 = RCCL).  Distinct devices
 * fall back to the same peer copies when librccl cannot be loaded or ncclCommInitAll fails. */
typedef struct hoh_mgpu hoh_mgpu;
int hoh_mgpu_create(hoh_mgpu** m, int ndev, const int* devices);
void hoh_mgpu_destroy(hoh_mgpu* m);
int hoh_mgpu_transport(const hoh_mgpu* m);
/* choh.cpp:394-527 over all devices: device r encodes a band of tile rows (choh.cpp:464-500) of
 * the host image h_rgb; one RCCL group gathers the blobs over xGMI behind hoh_file_prefix into
 * the file d_out on the first device.  Same bytes and printed size as hoh_encode_image. */
int hoh_mgpu_encode_image(hoh_mgpu* m, const uint8_t* h_rgb, int W, int H, int speed, uint8_t* d_out, size_t cap,
                          size_t* out_size, size_t* printed);
/* dhoh.cpp:297-396 over all devices: the file d_hoh (size bytes, on the first device) -> the host
 * image h_rgb (W*H*3 bytes, cap at least that).  The tile table is parsed on the host, one RCCL
 * group sends each device its tiles' bytes, each decodes its band. */
int hoh_mgpu_decode_image(hoh_mgpu* m, const uint8_t* d_hoh, size_t size, uint8_t* h_rgb, size_t cap, int* W,
                          int* H);

/* ---- entropy stream level (host buffers; one call = one stream, batched inside) --------- */

/* Replaces encode_entropy(uint16_t*, size_t, size_t, uint8_t*, uint32_t, uint8_t)
 * (entropy_encoding.hpp:8-15; u8 overload :283-290).  Same bytes; *written = stream bytes. */
int hoh_encode_entropy(hoh_ctx* ctx, const uint16_t* symbols, size_t n, size_t range,
                       uint32_t prob_bits, uint8_t* out, size_t cap, size_t* written);
size_t hoh_entropy_bound(size_t n, size_t range, uint32_t prob_bits);

/* Replaces decode_entropy(uint8_t*, size_t, size_t*, size_t*, uint8_t)
 * (entropy_decoding.hpp:134-140).  Advances *byte_pointer past the whole stream (Q1 fix);
 * *n = symbol count; out must hold cap symbols (hoh_entropy_count tells the count). */
int hoh_decode_entropy(hoh_ctx* ctx, const uint8_t* in, size_t in_size, size_t* byte_pointer,
                       uint16_t* out, size_t cap, size_t* n);
int hoh_entropy_count(const uint8_t* in, size_t in_size, size_t byte_pointer, size_t* n);

/* Framing of the stream at byte_pointer without decoding it (decode_entropy_simple,
 * entropy_decoding.hpp:8-132): header fields, where the frequency table ends, the rANS payload
 * size and where the whole stream ends (the Q1-corrected *byte_pointer).  Host only. */
typedef struct hoh_entropy_header {
  uint64_t range, count;               /* symbol range, symbol count (:143-144)               */
  uint32_t entropy_mode, prob_bits;    /* metadata byte (:151-154): 1 = rANS, 0 = stored       */
  uint32_t table_mode, symbol_bits;    /* table storage mode; bits per stored symbol (:146-149) */
  uint64_t table_end;                  /* offset after the frequency table (rANS streams)      */
  uint64_t payload_bytes;              /* rANS payload size (:256) or stored bytes             */
  uint64_t stream_end;                 /* offset after the whole stream                        */
} hoh_entropy_header;
int hoh_entropy_parse(const uint8_t* in, size_t in_size, size_t byte_pointer, hoh_entropy_header* h);

/* Batched device form: nstreams streams, stream i = d_syms[h_offsets[i] .. + h_counts[i]]
 * (h_offsets multiples of 8), all with the same range and prob_bits; stream i is written to
 * d_out + h_out_offsets[i] (caller-chosen, each with hoh_entropy_bound room); h_sizes[i]
 * receives its size. */
int hoh_encode_entropy_batch(hoh_ctx* ctx, const uint16_t* d_syms, const uint64_t* h_offsets,
                             const uint32_t* h_counts, int nstreams, uint32_t range,
                             uint32_t prob_bits, uint8_t* d_out, const uint64_t* h_out_offsets,
                             uint32_t* h_sizes, void* stream);

/* ---- plane level ------------------------------------------------------------------------ */

/* Replaces layer_encode(uint16_t*, size_t, int, int, int, size_t, uint8_t*, uint8_t*)
 * (layer_encode.hpp:11-20), cruncher_mode 0..4 (1..4: grid predictor search and prob_bits ladder,
 * with the reference's stale-prefix output; on a HOH_OPT_DECODABLE context the layer
 * hoh_layer_decode reads back).  nuke may be NULL (no LZ). */
int hoh_layer_encode(hoh_ctx* ctx, const uint16_t* data, size_t size, int width, int height,
                     int depth, size_t cruncher_mode, const uint8_t* nuke, uint8_t* out,
                     size_t cap, size_t* written);
/* Replaces decode_layer (layer_decode.hpp:128-136), returning the full-depth plane (u16: the
 * reference truncates 9-bit planes to u8).  Predictor-map layers use unpredict_all;
 * the -s0 MED layer uses MED on every row (Q9 fixed).  backref may be NULL. */
int hoh_layer_decode(hoh_ctx* ctx, const uint8_t* in, size_t in_size, size_t byte_pointer,
                     int width, int height, int depth, const uint16_t* backref, uint16_t* out);
/* Replaces channelpredict_fastpath (prediction.hpp:6-13; reached via channelpredict_section
 * :59-68): MED residuals. */
int hoh_predict_fastpath(hoh_ctx* ctx, const uint16_t* data, int width, int height, int depth,
                         uint16_t* out);
/* Replaces unpredict_all (unprediction.hpp:6-16) for the fast-path predictor (tile_map =
 * {0x0010}) with MED on every row (SURVEY Q9 fixed).  res holds nres residuals; backref may be
 * NULL. */
int hoh_unpredict_fastpath(hoh_ctx* ctx, const uint16_t* res, size_t nres, const uint16_t* backref,
                           int width, int height, int depth, uint16_t* out);
/* Replaces channelpredict_section (prediction.hpp:46-151): residuals of cell (cx, cy) of an
 * xt x yt grid with one predictor mask, in the cell's raster order; *count = residuals written
 * (out must hold the cell's pixel count). */
int hoh_predict_section(hoh_ctx* ctx, const uint16_t* data, int width, int height, int depth, int x_tiles,
                        int y_tiles, int x, int y, uint16_t predictor, uint16_t* out, size_t* count);
/* Replaces channelpredict_all (prediction.hpp:153-229): whole plane, one mask per grid cell. */
int hoh_predict_all(hoh_ctx* ctx, const uint16_t* data, int width, int height, int depth, int x_tiles,
                    int y_tiles, const uint16_t* tile_map, uint16_t* out);
/* Replaces unpredict_all (unprediction.hpp:6-91) for any predictor map: the exact inverse of
 * channelpredict_all with LZ copies (backref may be NULL).  A 1x1 {0x0010} map is the -s0 layer
 * and is inverted with MED on every row (SURVEY Q9 fixed), as hoh_unpredict_fastpath. */
int hoh_unpredict_all(hoh_ctx* ctx, const uint16_t* res, size_t nres, const uint16_t* backref, int width,
                      int height, int depth, int x_tiles, int y_tiles, const uint16_t* tile_map, uint16_t* out);
/* Replaces subtract_green (channel.hpp:73-79) and provides its inverse. */
int hoh_subtract_green(hoh_ctx* ctx, const uint8_t* rgb, size_t npix, uint16_t* G, uint16_t* R, uint16_t* B);
int hoh_add_green(hoh_ctx* ctx, const uint16_t* G, const uint16_t* R, const uint16_t* B, size_t npix, uint8_t* rgb);

/* ---- utilities ---------------------------------------------------------------------------- */

/* Deterministic synthetic RGB (hoh_ans/synth.py formula) written to d_rgb; _rows writes only
 * rows [y0, y0+rows) of a width-W image (a shard). */
int hoh_synth_rgb(hoh_ctx* ctx, uint8_t* d_rgb, int W, int H, uint64_t seed, int noise, void* stream);
int hoh_synth_rgb_rows(hoh_ctx* ctx, uint8_t* d_rgb, int W, int y0, int rows, uint64_t seed, int noise,
                       void* stream);
/* Natural-statistic synthetic RGB (hoh_ans/natural.py formula: piecewise-smooth regions, hard
 * edges, textures, flat runs, short repeats), rows [y0, y0+rows) of a width-W image. */
int hoh_natural_rgb_rows(hoh_ctx* ctx, uint8_t* d_rgb, int W, int y0, int rows, uint64_t seed, void* stream);

#ifdef __cplusplus
}
#endif
#endif
