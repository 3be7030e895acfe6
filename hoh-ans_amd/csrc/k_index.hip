// Decode side index capture (see include/hoh_ans.h, hoh_index): per stream, where its payload
// sits in the .hoh and the encoder checkpoints every HOH_SEG symbols.
#include "hoh_dec.h"

__global__ void k_index_capture(EncodeJob j, IndexStream* is, size_t per, int nstreams) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nstreams) return;
  const StreamInfo st = j.streams[s];
  IndexStream x;
  x.n = st.n;
  x.mode = st.mode;
  x.widx_end = st.widx_end;
  x.ckpt_off = (uint32_t)((size_t)s * per);       // the encoder's own checkpoint layout
  x.words = st.words;
  x.pad = 0;
  x.payload_off = st.out_off + st.hdr_len + hoh_varint_len((uint64_t)st.words * 4);
  // a stream the losing colour mode coded (k_layout: SK_I of a sub-green tile, the planes of a
  // palette tile) is not in the file: the decoder has no such stream, the index records none
  if (st.drop || st.n == 0) x.mode = SM_EMPTY;
  is[s] = x;
}

// Checkpoints of every rANS stream gathered into stream order (hoh_index_serialize, _concat):
// stream s's ceil(n / HOH_SEG) meaningful entries go to dst_off[s] .., their word index made
// relative to the stream's own payload.  rec12: the blob's 12-byte {xl, xh, wi} records, else
// Checkpoint.  One workgroup per stream.
__global__ __launch_bounds__(256) void k_index_pack(const IndexStream* is, const Checkpoint* ck, const uint32_t* dst_off,
                                                    void* dst, int rec12) {
  const IndexStream x = is[blockIdx.x];
  if (x.mode != SM_RANS) return;
  const uint32_t nseg = (x.n + HOH_SEG - 1) / HOH_SEG, o = dst_off[blockIdx.x];
  for (uint32_t k = threadIdx.x; k < nseg; k += blockDim.x) {
    const Checkpoint c = ck[(size_t)x.ckpt_off + k];
    const uint32_t wi = c.widx - x.widx_end;
    if (rec12) {
      uint32_t* p = (uint32_t*)dst + ((size_t)o + k) * 3;
      p[0] = c.xl; p[1] = c.xh; p[2] = wi;
    } else {
      Checkpoint q;
      q.xl = c.xl; q.xh = c.xh; q.widx = wi; q.pad = 0;
      ((Checkpoint*)dst)[(size_t)o + k] = q;
    }
  }
}

void launch_index_pack(const IndexStream* is, const Checkpoint* ck, const uint32_t* dst_off, int nstreams, void* dst,
                       int rec12, hipStream_t s) {
  if (nstreams > 0) hipLaunchKernelGGL(k_index_pack, dim3(nstreams), dim3(256), 0, s, is, ck, dst_off, dst, rec12);
}

void launch_index_capture(const EncodeJob& j, IndexStream* is, size_t per, hipStream_t s) {
  const int S = j.ntiles * SK_PER_TILE;
  hipLaunchKernelGGL(k_index_capture, dim3((S + 255) / 256), dim3(256), 0, s, j, is, per, S);
}

void dec_free(DecWork& w) {
  noix_release(w);
  for (int i = 0; i < HOH_DEC_NBUF; i++) {
    if (w.bufs[i]) (void)hipFree(w.bufs[i]);
    w.bufs[i] = nullptr;
    w.sizes[i] = 0;
  }
}
