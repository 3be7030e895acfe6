// One wave moves one row of nb bytes between two byte addresses of any alignment (k_dcrop,
// k_mgather, k_mscatter).  Source and destination that agree mod 16 get 16-byte moves between a
// byte head and tail; otherwise the destination still gets aligned dword stores, each assembled
// with v_alignbyte from the two aligned source dwords that hold its four bytes.
// Only bytes [0, nb) of d are written: rows that share dwords with their neighbours (packed images)
// stay whole.  Every load is a byte of the row, or an aligned dword / uint4 that holds at least one
// byte of the row (a body unit lies wholly inside the row, and with a source shift sh != 0 both
// dwords around it carry some of its bytes), so no load can leave the allocation the row lives in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ void wave_move_row(const uint8_t* s, uint8_t* d, uint32_t nb, int lane) {
  const uint32_t wide = (((uintptr_t)s ^ (uintptr_t)d) & 15) == 0 ? 16u : 4u;
  uint32_t head = (uint32_t)(-(intptr_t)d) & (wide - 1);      // bytes up to the destination's alignment
  if (head > nb) head = nb;
  const uint32_t body = (nb - head) / wide;                   // aligned units
  const uint32_t tail0 = head + body * wide;
  if ((uint32_t)lane < head) d[lane] = s[lane];
  if ((uint32_t)lane < nb - tail0) d[tail0 + lane] = s[tail0 + lane];
  if (wide == 16) {
    const uint4* s4 = (const uint4*)(s + head);
    uint4* d4 = (uint4*)(d + head);
    for (uint32_t i = lane; i < body; i += 64) d4[i] = s4[i];
  } else {
    const uint8_t* sb = s + head;
    const uint32_t sh = (uint32_t)((uintptr_t)sb & 3);
    const uint32_t* sw = (const uint32_t*)(sb - sh);
    uint32_t* d1 = (uint32_t*)(d + head);
    if (sh == 0) {
      for (uint32_t i = lane; i < body; i += 64) d1[i] = sw[i];
    } else {
      for (uint32_t i = lane; i < body; i += 64) d1[i] = __builtin_amdgcn_alignbyte(sw[i + 1], sw[i], sh);
    }
  }
}
