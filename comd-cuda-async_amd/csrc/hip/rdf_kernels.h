// rdf_kernels.h -- the pair-distance histogram behind g(r) for gfx950 (computePairHistogram, comd_hip.h).  The reference has no counterpart.
//
//   counts[k] = number of ordered pairs (i local, j local or halo, j != i) with k dr <= r_ij < (k + 1) dr,   dr = rMax / nBins, k < nBins
// Only local atoms are i and j runs over local and halo slots, so every unordered pair is counted once from each side (on two ranks when it
// straddles a rank boundary): the sum over ranks is twice the number of unordered pairs.
//
// Mapping: the one of Virial_thread_atom (virial_kernels.h).  One wave = one 64-slot chunk of a local cell (a cell of more than 64 slots takes
// several chunks), lane = i atom, the 27-cell stencil walked with the neighbour j wave-uniform through the scalar load stream, 8 per batch.  A
// chunk of at most 32 atoms -- every EAM cell, LJ at 2.5 sigma, the tail chunk of an LJ cell -- is replicated across the lanes, each copy
// walking a share of the stencil cells.  Each workgroup takes a contiguous run of chunks, dealt XCD-contiguously (xcdRemap).
// The link cells of the *_nl methods and of -L are sized for cutoff + skin and are not re-binned between list builds: an atom has moved less
// than skin/2 since, so two atoms within the plain cutoff now were within cutoff + skin of each other when the cells were filled, i.e. in
// neighbouring cells.  With rMax <= the force cutoff (the host refuses anything else) the 27-cell walk therefore sees every pair.
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
#include "device_common.h"

#define PAIRHIST_MAX_BINS 4096         // 4 waves x 4096 bins x 4 bytes = 64 KiB of LDS
#define PAIRHIST_BLOCKS 2048

struct PairHistArgs {
   const real_t* __restrict__ rx; const real_t* __restrict__ ry; const real_t* __restrict__ rz;
   const int* __restrict__ nAtoms;
   const int* __restrict__ nbr;        // [nLocal*27], self first
   int nLocalBoxes, cap, chunks;       // chunks = 64-slot chunks per cell
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

   const long nWork = (long)v.nLocalBoxes * v.chunks;
   const long per = (nWork + gridDim.x - 1) / gridDim.x;
   const long w0 = (long)xcdRemap(blockIdx.x, gridDim.x) * per;
   const long w1 = w0 + per < nWork ? w0 + per : nWork;
   for (long w = w0 + wave; w < w1; w += 4) {
      const int iBox = uniform((int)(w / v.chunks));
      const int first = uniform((int)(w - (long)iBox * v.chunks)) * WAVE;
      const int ni = uniform(v.nAtoms[iBox]);
      if (first >= ni) continue;
      // a chunk of m <= 32 atoms is replicated: reps copies of its atoms, copy q walks the stencil cells q, q + reps, ... (as Virial_thread_atom)
      const int m = ni - first < WAVE ? ni - first : WAVE;
      int reps = 1;
      while (reps < 16 && 2 * reps * m <= WAVE) reps *= 2;
      const int span = WAVE / reps, q = lane / span;
      const int ia = first + (lane & (span - 1));
      const bool active = ia < first + m;
      const size_t iOff = (size_t)iBox * v.cap + (active ? ia : first);
      const real_t xi = v.rx[iOff], yi = v.ry[iOff], zi = v.rz[iOff];
      auto test = [&](real_t xj, real_t yj, real_t zj) {
         const real_t dx = xi - xj, dy = yi - yj, dz = zi - zj;
         const real_t r2 = dx*dx + dy*dy + dz*dz;
         if (active && r2 < v.rMax2 && r2 > R(0.0)) {
            int bin = (int)(r2 * rsqrtR(r2) * v.invDr);       // r / dr; a round-up of r at the last edge stays in the last bin
            bin = bin < top ? bin : top;
            atomicAdd(mine + bin, 1u);
         }
      };
      const int* __restrict__ nb = v.nbr + (size_t)iBox * 27;
      if (reps > 1) {
         for (int k = q; k < 27; k += reps) {
            const int jBox = nb[k];
            const int nj = v.nAtoms[jBox];
            const size_t base = (size_t)jBox * v.cap;
            for (int j = 0; j < nj; ++j) test(v.rx[base + j], v.ry[base + j], v.rz[base + j]);
         }
      } else for (int k = 0; k < 27; ++k) {
         const int jBox = uniform(nb[k]);
         const int nj = uniform(v.nAtoms[jBox]);
         const size_t base = (size_t)jBox * v.cap;
         const real_t* __restrict__ qx = v.rx + base;
         const real_t* __restrict__ qy = v.ry + base;
         const real_t* __restrict__ qz = v.rz + base;
         int j = 0;
         for (; j + 8 <= nj; j += 8) {
            real_t xs[8], ys[8], zs[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { xs[u] = qx[j + u]; ys[u] = qy[j + u]; zs[u] = qz[j + u]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) test(xs[u], ys[u], zs[u]);
         }
         for (; j < nj; ++j) test(qx[j], qy[j], qz[j]);
      }
   }
   __syncthreads();
   // bin k of the workgroup = the sum of its 4 copies; a crystal leaves most bins empty
   for (int k = threadIdx.x; k < v.nBins; k += 256) {
      unsigned long long sum = 0ull;
      for (int wv = 0; wv < 4; ++wv) sum += sHist[wv * v.nBins + k];
      if (sum) atomicAdd(v.counts + k, sum);
   }
}
