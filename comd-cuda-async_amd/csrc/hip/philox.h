/* philox.h -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11), counter-based:
 * the four output words are a pure function of a 128-bit counter and a 64-bit key, so a stream needs no state.  The Langevin thermostat
 * (langevin_kernels.h) keys it with the run's seed and counts with (atom gid, global step): the noise an atom receives does not depend on
 * the slot, cell, method or rank that holds it.  Plain C and HIP alike (the device kernels and the host test program include it). */
#ifndef COMD_PHILOX_H
#define COMD_PHILOX_H

#include <stdint.h>

#if defined(__HIPCC__)
#define COMD_PHILOX_FN __host__ __device__ __forceinline__
#else
#define COMD_PHILOX_FN static inline
#endif

#define COMD_PHILOX_M0 0xD2511F53u
#define COMD_PHILOX_M1 0xCD9E8D57u
#define COMD_PHILOX_W0 0x9E3779B9u
#define COMD_PHILOX_W1 0xBB67AE85u

/* ctr[4] in, out[4] out; key = {k0, k1}.  Ten rounds, the key bumped by the Weyl constants between them (Random123 philox4x32_R(10)). */
COMD_PHILOX_FN void comdPhilox4x32_10(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4])
{
   uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
   for (int r = 0; r < 10; ++r) {
      if (r > 0) { k0 += COMD_PHILOX_W0; k1 += COMD_PHILOX_W1; }
      const uint64_t p0 = (uint64_t)COMD_PHILOX_M0 * c0, p1 = (uint64_t)COMD_PHILOX_M1 * c2;
      const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
      c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
   }
   out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

#endif
