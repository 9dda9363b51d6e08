// rdf_kernels.h -- the pair-distance histogram behind g(r) for gfx950 (computePairHistogram, comd_hip.h).  The reference has no counterpart.
//
//   counts[k] = number of ordered pairs (i local, j local or halo, j != i) with k dr <= r_ij < (k + 1) dr,   dr = rMax / nBins, k < nBins
// Only local atoms are i and j runs over local and halo slots, so every unordered pair is counted once from each side (on two ranks when it
// straddles a rank boundary): the sum over ranks is twice the number of unordered pairs.
//
// Mapping: the chunk walk of stencil_walk.h, which also says why 27 cells are enough for the cells of the *_nl methods and of -L as long as
// rMax <= the force cutoff (the host refuses anything else).
//
// Counters: every lane bins its own pair, so this is a scattered histogram, not a reduction.  Each workgroup keeps 32-bit counters in
// dynamic LDS, private to it, one copy per wave ([wave][bin]).  The lanes of one ds_add that meet in a bin queue on its address -- on a crystal
// nearly all of them do -- but at 80^3 the step-0 lattice costs what the thermal state costs (LJ 6.1 against 6.2 ms, EAM 1.95 against 1.84 ms,
// DESIGN.md section 3), so there are no lane-striped copies and no wave-level pre-aggregation of equal bins.  At the end the workgroup adds its four copies up and flushes the non-zero bins with one
// 64-bit global atomicAdd each into a buffer the host has zeroed on the same stream.  Sums of integers do not depend on the order of arrival:
// the result is bit-reproducible as it stands, without the fixed-order partial rows the virial's floating-point sums need.
// A 32-bit LDS counter cannot overflow: a workgroup walks `per` chunks, each adds at most 64 lanes x 27 cells x cap slots to all counters of
// a wave together, and the host sizes the grid so that per x 64 x 27 x cap < 2^32 (computePairHistogram: the fixed 2048 workgroups hold up
// to 256^3 LJ cells at 5 sigma -- 493,039 cells x 3 chunks / 2048 = 723 chunks x 64 x 27 x 192 = 2.4e8 -- and beyond it the grid grows, which
// changes nothing in a sum of integers).
//
// The kernel reads r, nAtoms and nbr and writes nothing but its own buffer.
#pragma once
#include "stencil_walk.h"

#define PAIRHIST_MAX_BINS 4096         // 4 waves x 4096 bins x 4 bytes = 64 KiB of LDS
#define PAIRHIST_BLOCKS 2048

struct PairHistArgs : StencilArgs {
   int nBins;
   real_t rMax2, invDr;                // rMax^2, nBins / rMax
   unsigned long long* __restrict__ counts;      // [nBins], zeroed before the launch
};

__global__ __launch_bounds__(256)
void PairHist_thread_atom(PairHistArgs v)
{
   extern __shared__ unsigned sHist[];            // [4 waves][nBins]
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;
   for (int k = threadIdx.x; k < 4 * v.nBins; k += 256) sHist[k] = 0u;
   __syncthreads();
   unsigned* __restrict__ mine = sHist + wave * v.nBins;
   const int top = v.nBins - 1;

   forEachChunk(v, lane, wave, [&](int iBox, int first, int, int reps, int, int q, int ia, bool active) {
      const size_t iOff = (size_t)iBox * v.cap + (active ? ia : first);
      const real_t xi = v.rx[iOff], yi = v.ry[iOff], zi = v.rz[iOff];
      auto test = [&](real_t xj, real_t yj, real_t zj, size_t) {
         const real_t dx = xi - xj, dy = yi - yj, dz = zi - zj;
         const real_t r2 = dx*dx + dy*dy + dz*dz;
         if (active && r2 < v.rMax2 && r2 > R(0.0)) {
            int bin = (int)(r2 * rsqrtR(r2) * v.invDr);       // r / dr; a round-up of r at the last edge stays in the last bin
            bin = bin < top ? bin : top;
            atomicAdd(mine + bin, 1u);
         }
      };
      stencilWalk<size_t>(v, iBox, reps, q, test);
   });
   __syncthreads();
   // bin k of the workgroup = the sum of its 4 copies; a crystal leaves most bins empty
   for (int k = threadIdx.x; k < v.nBins; k += 256) {
      unsigned long long sum = 0ull;
      for (int wv = 0; wv < 4; ++wv) sum += sHist[wv * v.nBins + k];
      if (sum) atomicAdd(v.counts + k, sum);
   }
}
