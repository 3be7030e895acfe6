// Predictor primitives shared by the encoder search (k_search.hip) and the decoder (k_decode.hip):
// the 16 predictors of prediction.hpp:116-133 / :190-207, the lane-varying pick and the first
// masked predictor of least error.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>


__device__ __forceinline__ uint32_t med16s(uint32_t a, uint32_t b, uint32_t c) {   // predictor_operations.hpp:37-60
  if (a > b) return b > c ? b : (c > a ? a : c);
  return b < c ? b : (c > a ? c : a);
}
__device__ __forceinline__ uint32_t midp(uint32_t a, uint32_t b) {                 // :8-10
  // a + (b - a) / 2 (truncated) == (a + b + (b < a)) / 2 for a, b < 2^31 (every value here is u16)
  return (a + b + (b < a ? 1u : 0u)) >> 1;
}
__device__ __forceinline__ uint32_t avg3(uint32_t a, uint32_t b, uint32_t c) { return (a + b + c) / 3; }   // :66-68
__device__ __forceinline__ uint32_t paeth(int A, int B, int C) {                   // :89-106
  const int p = A + B - C;
  const int Ap = abs(A - p), Bp = abs(B - p), Cp = abs(C - p);
  if (Ap < Bp) return Ap < Cp ? A : C;
  return Bp < Cp ? B : C;
}

struct Preds { uint32_t v[16]; };

// prediction.hpp:116-133 (section: paeth(L, T, TL)) / :190-207 (all: paeth(L, TL, T))
__device__ __forceinline__ void preds16(uint32_t L, uint32_t T, uint32_t TL, uint32_t TR, bool all, Preds& p) {
  p.v[0] = L; p.v[1] = T; p.v[2] = TL; p.v[3] = TR;
  p.v[4] = med16s(T, L, (T + L - TL) & 0xffffu);
  p.v[5] = midp(L, T); p.v[6] = midp(L, TL); p.v[7] = midp(TL, T); p.v[8] = midp(T, TR);
  p.v[9] = all ? paeth(L, TL, T) : paeth(L, T, TL);
  p.v[10] = avg3(L, L, TL); p.v[11] = avg3(L, TL, TL); p.v[12] = avg3(TL, TL, T);
  p.v[13] = avg3(TL, T, T); p.v[14] = avg3(T, T, TR); p.v[15] = avg3(T, TR, TR);
}

// p.v[k] for a lane-varying k without dynamic register indexing: a 4-level tree of bit blends
// (v_bfi_b32). The masks pass through an empty asm so the compiler cannot see they are 0 / ~0:
// written as selects, it folded the tree into a dynamically indexed private array (Preds and the
// tree levels in scratch, ~12 dependent scratch round trips per pixel step of the cell walk).
__device__ __forceinline__ uint32_t blend(uint32_t a, uint32_t b, uint32_t m) { return (a & ~m) | (b & m); }
__device__ __forceinline__ uint32_t pick(const Preds& p, uint32_t k) {
  uint32_t m0 = 0u - (k & 1u), m1 = 0u - ((k >> 1) & 1u), m2 = 0u - ((k >> 2) & 1u), m3 = 0u - ((k >> 3) & 1u);
  asm volatile("" : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3));
  const uint32_t a0 = blend(p.v[0], p.v[1], m0), a1 = blend(p.v[2], p.v[3], m0), a2 = blend(p.v[4], p.v[5], m0),
                 a3 = blend(p.v[6], p.v[7], m0), a4 = blend(p.v[8], p.v[9], m0), a5 = blend(p.v[10], p.v[11], m0),
                 a6 = blend(p.v[12], p.v[13], m0), a7 = blend(p.v[14], p.v[15], m0);
  const uint32_t b0 = blend(a0, a1, m1), b1 = blend(a2, a3, m1), b2 = blend(a4, a5, m1), b3 = blend(a6, a7, m1);
  return blend(blend(b0, b1, m2), blend(b2, b3, m2), m3);
}

// first masked predictor of least |v - p| (prediction.hpp:138-146, :213-224)
// (the smallest key (|v - p_k| << 4) | k over the masked k: |v - p_k| < 2^16 < 2c never fails the
// reference's d < 2c test)
__device__ __forceinline__ uint32_t best_pred(uint32_t v, const Preds& p, uint32_t mask, int c) {
  (void)c;
  uint32_t best = 0xffffffffu;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint32_t key = (__builtin_amdgcn_sad_u16(v, p.v[k], 0u) << 4) | (uint32_t)k;
    best = min(best, ((mask >> k) & 1) ? key : 0xffffffffu);
  }
  return best & 15u;
}
