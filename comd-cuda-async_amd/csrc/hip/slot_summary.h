// slot_summary.h -- the two-stage summary over the occupied slots of per-atom planes: AtomStress_Summary / AtomStress_SummaryFinal (stress_kernels.h)
// and AtomStrain_Summary / AtomStrain_SummaryFinal (strain_kernels.h).  The reference has no counterpart.
//
// A record type SUM holds one candidate -- doubles and ints, its size a multiple of 4 bytes -- and supplies
//   static SUM empty()               the neutral candidate
//   void join(const SUM& b)          symmetric in its operands (a + b, the extremes, the lower gid): both sides of a pair end with the same bits
//   static const int N               the doubles of a row
//   void toRow(double* row) const    gids and counts as doubles: exact
//   static SUM fromRow(const double* row)
// Stage 1: a fixed grid walks the slots with a fixed stride, every thread joins the candidates of its occupied slots, the workgroup joins in a fixed
// order and writes one row.  Stage 2: one workgroup joins the rows the same way.  The order of the joins: the butterfly over the lanes (m = 32 ... 1),
// then the waves 1, 2, 3 onto wave 0 on thread 0.  No atomics: bit-reproducible.
#pragma once
#include "device_common.h"

// the record of lane addr / 4, moved one dword at a time
template <class SUM>
__device__ __forceinline__ SUM bpermuteRecord(const SUM& a, int addr)
{
   static_assert(sizeof(SUM) % sizeof(int) == 0, "a summary record is moved in dwords");
   int w[sizeof(SUM) / sizeof(int)];
   __builtin_memcpy(w, &a, sizeof(SUM));
#pragma unroll
   for (unsigned k = 0; k < sizeof(SUM) / sizeof(int); ++k) w[k] = __builtin_amdgcn_ds_bpermute(addr, w[k]);
   SUM b;
   __builtin_memcpy(&b, w, sizeof(SUM));
   return b;
}

// over the 64 lanes, then over the 4 waves, in a fixed order; thread 0 ends with the workgroup's candidate
template <class SUM>
__device__ __forceinline__ void summaryBlockJoin(SUM& a)
{
   __shared__ SUM sWave[4];
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;
#pragma unroll
   for (int m = 32; m >= 1; m >>= 1) a.join(bpermuteRecord(a, (lane ^ m) << 2));
   if (lane == 0) sWave[wave] = a;
   __syncthreads();
   if (threadIdx.x == 0)
      for (int w = 1; w < 4; ++w) a.join(sWave[w]);
}

// stage 1: candidate(o) of the occupied slots o < nSlots -> one row per workgroup, partial[blockIdx.x][SUM::N]
template <class SUM, class CANDIDATE>
__device__ __forceinline__ void summaryOfSlots(size_t nSlots, const int* __restrict__ nAtoms, int cap, double* __restrict__ partial, CANDIDATE candidate)
{
   SUM a = SUM::empty();
   for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < nSlots; o += (size_t)gridDim.x * blockDim.x) {
      const size_t b = o / (size_t)cap;
      if ((int)(o - b * (size_t)cap) >= nAtoms[b]) continue;
      a.join(candidate(o));
   }
   summaryBlockJoin(a);
   if (threadIdx.x == 0) a.toRow(partial + (size_t)blockIdx.x * SUM::N);
}

// stage 2: the rows -> out[SUM::N]
template <class SUM>
__device__ __forceinline__ void summaryOfRows(const double* __restrict__ partial, int nPartial, double* __restrict__ out)
{
   SUM a = SUM::empty();
   for (int i = threadIdx.x; i < nPartial; i += blockDim.x) a.join(SUM::fromRow(partial + (size_t)i * SUM::N));
   summaryBlockJoin(a);
   if (threadIdx.x == 0) a.toRow(out);
}
