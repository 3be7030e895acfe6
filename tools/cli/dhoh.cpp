// dhoh drop-in (dhoh.cpp:297-420): `dhoh in.hoh out.rgb` on the GPU.  Decodes tiled RGB .hoh
// files as written by choh -s0 (the reference crashes on them) and writes the raw
// interleaved RGB bytes.  Return codes: 3/4 not a .hoh, 5 unknown pixel format, and the
// library's status code for anything it cannot decode.  `--gpus N` / `--devices a,b,..`
// (tools/cli/gpus.h) decode over several GPUs in this process (hoh_mgpu_decode_image).
// After the reference's arguments (one GPU only): `--index in.hix` decodes with the side index in
// that sidecar (hoh_index_deserialize; choh --index or dhoh --write-index wrote it);
// `--write-index out.hix` builds the index from the file (hoh_index_build), writes it and decodes
// with it -- for a file the builder does not cover it writes the empty index and decodes without.
// The context always has HOH_OPT_SMALL_IMAGES set: a file of at most 511 x 511 that carries its tile
// (choh --small-images) decodes; the reference's header-only file is refused as before.
// `--region x,y,w,h` (one GPU, with or without the index options) decodes only the tiles that
// window touches (hoh_decode_region) and writes its w*h*3 bytes; a malformed region or one not
// inside the image prints the usage line and returns 1.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/hoh_ans.h"
#include "gpus.h"

int main(int argc, char** argv) {
  const char *hix_in = nullptr, *hix_out = nullptr, *region = nullptr;
  static const char* usage = "usage: dhoh infile.hoh outfile.rgb [--index in.hix] [--write-index out.hix] [--region x,y,w,h]\n";
  {
    int w = 1;
    for (int i = 1; i < argc; i++) {
      if (!std::strcmp(argv[i], "--index") && i + 1 < argc) hix_in = argv[++i];
      else if (!std::strcmp(argv[i], "--write-index") && i + 1 < argc) hix_out = argv[++i];
      else if (!std::strcmp(argv[i], "--region") && i + 1 < argc) region = argv[++i];
      else argv[w++] = argv[i];
    }
    argc = w;
  }
  const std::vector<int> devices = take_devices(argc, argv);
  if ((hix_in || hix_out) && devices.size() > 1) {
    std::printf("--index / --write-index decode on one GPU\n");
    return 1;
  }
  int rx = 0, ry = 0, rw = 0, rh = 0;
  if (region) {
    char extra = 0;
    if (std::sscanf(region, "%d,%d,%d,%d%c", &rx, &ry, &rw, &rh, &extra) != 4 || rx < 0 || ry < 0 || rw <= 0 || rh <= 0) {
      std::printf("bad region '%s'\n%s", region, usage);
      return 1;
    }
    if (devices.size() > 1) {
      std::printf("--region decodes on one GPU\n");
      return 1;
    }
  }
  if (argc == 2 && (!std::strcmp(argv[1], "--help") || !std::strcmp(argv[1], "-h"))) {
    std::printf("usage: dhoh infile.hoh outfile.rgb\n");
    return 0;
  }
  if (argc == 2 && !std::strcmp(argv[1], "--version")) { std::printf("%s\n", hoh_version()); return 0; }
  if (argc < 3) { std::printf("not enough arguments!\nusage: dhoh infile.hoh outfile.rgb\n"); return 1; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("could not read %s\n", argv[1]); return 3; }
  std::vector<uint8_t> in;
  {
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    in.resize(n > 0 ? (size_t)n : 0);
    if (!in.empty() && std::fread(in.data(), 1, in.size(), f) != in.size()) { std::fclose(f); return 3; }
    std::fclose(f);
  }
  if (in.size() < 8) { std::printf("not a valid hoh file!\n"); return 3; }
  if (in[0] != 153 || in[1] != 72 || in[2] != 79 || in[3] != 72) { std::printf("not a valid hoh file!\n"); return 4; }
  static const char* fmt[] = {"bit", "greyscale", "rgb", "greyscale + alpha", "rgb + alpha"};
  if (in[4] <= 4) std::printf("pixel format: %s\n", fmt[in[4]]);
  else if (in[4] == 255) { std::printf("invalid pixel format!\n"); return 4; }
  else { std::printf("unknown pixel format!\n"); return 5; }
  int W = 0, H = 0, xt = 0, yt = 0;
  int r = hoh_peek_header(in.data(), in.size(), &W, &H, &xt, &yt);
  if (r != HOH_OK) { std::fprintf(stderr, "dhoh: %s\n", hoh_strerror(r)); return r; }
  std::printf("width: %d\nheight: %d\n", W, H);
  if (region && (rx > W - rw || ry > H - rh)) {
    std::printf("region '%s' is not inside the image\n%s", region, usage);
    return 1;
  }
  hoh_ctx* ctx = nullptr;
  const int dev0 = devices.empty() ? 0 : devices[0];   // --devices 3 / one entry: that GPU
  hoh_mgpu* mg = nullptr;
  r = devices.size() > 1 ? hoh_mgpu_create(&mg, (int)devices.size(), devices.data()) : hoh_ctx_create(&ctx, dev0);
  if (r == HOH_OK && ctx) r = hoh_ctx_set_option(ctx, HOH_OPT_SMALL_IMAGES, 1);
  if (r != HOH_OK) { std::fprintf(stderr, "dhoh: %s\n", hoh_strerror(r)); return r; }
  const size_t raw = region ? (size_t)rw * rh * 3 : (size_t)W * H * 3;
  uint8_t *d_in = nullptr, *d_rgb = nullptr;
  (void)hipSetDevice(dev0);
  if (hipMalloc(&d_in, in.size()) != hipSuccess || (!mg && hipMalloc(&d_rgb, raw) != hipSuccess)) return HOH_E_HIP;
  if (hipMemcpy(d_in, in.data(), in.size(), hipMemcpyHostToDevice) != hipSuccess) return HOH_E_HIP;
  std::vector<uint8_t> out(raw);
  if (mg) {
    r = hoh_mgpu_decode_image(mg, d_in, in.size(), out.data(), raw, &W, &H);
  } else {
    hoh_index* ix = nullptr;
    if (hix_in || hix_out) {
      if ((r = hoh_index_create(&ix)) != HOH_OK) { std::fprintf(stderr, "dhoh: %s\n", hoh_strerror(r)); return r; }
    }
    if (hix_in) {
      std::vector<uint8_t> blob;
      FILE* xf = std::fopen(hix_in, "rb");
      if (!xf) { std::printf("could not read %s\n", hix_in); return 3; }
      std::fseek(xf, 0, SEEK_END);
      const long bn = std::ftell(xf);
      std::fseek(xf, 0, SEEK_SET);
      blob.resize(bn > 0 ? (size_t)bn : 0);
      const bool got = blob.empty() || std::fread(blob.data(), 1, blob.size(), xf) == blob.size();
      std::fclose(xf);
      if (!got) { std::printf("could not read %s\n", hix_in); return 3; }
      r = hoh_index_deserialize(ix, blob.data(), blob.size(), nullptr);
      if (r != HOH_OK) { std::fprintf(stderr, "dhoh: %s: %s\n", hix_in, hoh_strerror(r)); return r; }
    }
    if (hix_out) {
      int bw = 0, bh = 0;
      r = hoh_index_build(ctx, d_in, in.size(), ix, &bw, &bh, nullptr);
      if (r != HOH_OK && r != HOH_E_UNSUPPORTED) { std::fprintf(stderr, "dhoh: %s\n", hoh_strerror(r)); return r; }
      std::vector<uint8_t> blob(hoh_index_serialized_size(ix));   // the empty index when unsupported
      size_t bn = 0;
      r = hoh_index_serialize(ix, blob.data(), blob.size(), &bn, hoh_ctx_stream(ctx));
      if (r != HOH_OK) { std::fprintf(stderr, "dhoh: %s\n", hoh_strerror(r)); return r; }
      FILE* xf = std::fopen(hix_out, "wb");
      if (!xf || std::fwrite(blob.data(), 1, bn, xf) != bn) { std::printf("could not write %s\n", hix_out); return 3; }
      std::fclose(xf);
    }
    if (region) r = hoh_decode_region(ctx, d_in, in.size(), rx, ry, rw, rh, d_rgb, (size_t)rw * 3, raw, &W, &H, ix, nullptr);
    else r = hoh_decode_image_ix(ctx, d_in, in.size(), d_rgb, raw, &W, &H, ix, nullptr);
    if (ix) hoh_index_destroy(ix);
    if (r == HOH_OK && hipMemcpy(out.data(), d_rgb, raw, hipMemcpyDeviceToHost) != hipSuccess) r = HOH_E_HIP;
  }
  if (r != HOH_OK) { std::fprintf(stderr, "dhoh: %s\n", hoh_strerror(r)); return r; }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(out.data(), 1, raw, o) != raw) { std::printf("could not write %s\n", argv[2]); return 3; }
  std::fclose(o);
  (void)hipFree(d_in);
  if (d_rgb) (void)hipFree(d_rgb);
  if (mg) hoh_mgpu_destroy(mg);
  if (ctx) hoh_ctx_destroy(ctx);
  return 0;
}
