// stencil_walk.h -- the mapping of the analysis kernels onto the link cells: Virial_thread_atom (virial_kernels.h), PairHist_thread_atom
// (rdf_kernels.h), CentroSym_thread_atom (csp_kernels.h) and Cna_thread_atom (cna_kernels.h).  The reference has no counterpart.
//
// Mapping.  The unit of work is one 64-slot chunk of a local cell (a cell of more than 64 slots takes several chunks).  Each workgroup of 4 waves takes
// a contiguous run of chunks -- neighbouring cells share stencil cells -- dealt XCD-contiguously (xcdRemap); its waves interleave, one wave per chunk,
// lane = atom i.  A full chunk walks the 27 stencil cells with the neighbour j wave-uniform: positions through the scalar unit, 8 per batch of loads,
// then their tests (the shape of ljCellLoop).  A chunk of m <= 32 atoms -- every EAM cell, LJ at 2.5 sigma, the tail chunk of an LJ cell -- would use
// half the lanes or fewer, so it is replicated: reps copies of its atoms (the largest power of two <= 16 with reps * m <= 64), copy q walks the
// stencil cells q, q + reps, ...  The neighbour then differs between the copies: per-lane loads instead of the scalar stream.  What a kernel does
// with the copies' partial results is its own business (sums and counts need nothing; the 12-nearest sets are merged, nearest12_walk.h).
// Only local atoms are i, j runs over local and halo slots: every pair is seen from both sides (on two ranks when it straddles a rank boundary).
//
// Why 27 cells are enough.  The link cells of the *_nl methods and of -L are sized for cutoff + skin and are not re-binned between list builds: an
// atom has moved less than skin/2 since, so two atoms within the plain cutoff now were within cutoff + skin of each other when the cells were filled,
// i.e. in neighbouring cells.  The 27-cell walk with a radius <= the plain cutoff (the hosts refuse anything else) therefore sees every pair, the
// ones the lists hold included.
//
// The helpers take the kernel's text as lambdas and hand it values, not references: forEachChunk filling a record by reference cost Cna_thread_atom 8
// bytes of scratch and the others 2 to 4 VGPRs.
#pragma once
#include "device_common.h"

// what every user of the walk reads; its argument record derives from this
struct StencilArgs {
   const real_t* __restrict__ rx; const real_t* __restrict__ ry; const real_t* __restrict__ rz;
   const int* __restrict__ nAtoms;
   const int* __restrict__ nbr;        // [nLocal*27], self first
   int nLocalBoxes, cap, chunks;       // chunks = 64-slot chunks per cell
};

// body(iBox, first, m, reps, span, q, ia, active) for every non-empty chunk of the wave: cell, first slot of the chunk, its atoms, the copies, the
// lanes of a copy, the lane's copy, the lane's slot in the cell, and whether that slot holds an atom (an idle lane computes on slot `first`)
template <class BODY>
__device__ __forceinline__ void forEachChunk(const StencilArgs& v, int lane, int wave, BODY body)
{
   const long nWork = (long)v.nLocalBoxes * v.chunks;
   const long per = (nWork + gridDim.x - 1) / gridDim.x;
   const long w0 = (long)xcdRemap(blockIdx.x, gridDim.x) * per;
   const long w1 = w0 + per < nWork ? w0 + per : nWork;
   for (long w = w0 + wave; w < w1; w += 4) {
      const int iBox = uniform((int)(w / v.chunks));
      const int first = uniform((int)(w - (long)iBox * v.chunks)) * WAVE;
      const int ni = uniform(v.nAtoms[iBox]);
      if (first >= ni) continue;
      const int m = ni - first < WAVE ? ni - first : WAVE;
      int reps = 1;
      while (reps < 16 && 2 * reps * m <= WAVE) reps *= 2;
      const int span = WAVE / reps, q = lane / span;
      const int ia = first + (lane & (span - 1));
      const bool active = ia < first + m;
      body(iBox, first, m, reps, span, q, ia, active);
   }
}

// The shares of the copies of a replicated chunk into one, for sums and counts (real_t, double or int): after the doubling over s every lane holds the
// sum over the copies lane ^ s, lane ^ 2s, ... as well.  a + b is what both lanes of a pair compute, so every copy ends with the same bits, in an
// order that depends on reps alone.  One loop over s with all values inside it: one address serves them all.
template <class... T>
__device__ __forceinline__ void sumOverCopies(int lane, int span, T&... x)
{
   for (int s = span; s < WAVE; s <<= 1) {
      const int addr = (lane ^ s) << 2;
      ((x += bpermuteAddrR(x, addr)), ...);
   }
}

// test(xj, yj, zj, slot) for the slots of the stencil cells of iBox: copy q's share of them when the chunk is replicated, else all 27 with the
// neighbour wave-uniform.  IDX: the type slots are computed in (size_t, or int where the host has checked that they fit)
template <class IDX, class TEST>
__device__ __forceinline__ void stencilWalk(const StencilArgs& v, int iBox, int reps, int q, TEST test)
{
   const int* __restrict__ nb = v.nbr + (size_t)iBox * 27;
   if (reps > 1) {
      for (int k = q; k < 27; k += reps) {
         const int jBox = nb[k];
         const int nj = v.nAtoms[jBox];
         const IDX base = (IDX)jBox * v.cap;
         for (int j = 0; j < nj; ++j) test(v.rx[base + j], v.ry[base + j], v.rz[base + j], base + j);
      }
   } else for (int k = 0; k < 27; ++k) {
      const int jBox = uniform(nb[k]);
      const int nj = uniform(v.nAtoms[jBox]);
      const IDX base = (IDX)jBox * v.cap;
      const real_t* __restrict__ qx = v.rx + base;
      const real_t* __restrict__ qy = v.ry + base;
      const real_t* __restrict__ qz = v.rz + base;
      int j = 0;
      for (; j + 8 <= nj; j += 8) {
         real_t xs[8], ys[8], zs[8];
#pragma unroll
         for (int u = 0; u < 8; ++u) { xs[u] = qx[j + u]; ys[u] = qy[j + u]; zs[u] = qz[j + u]; }
#pragma unroll
         for (int u = 0; u < 8; ++u) test(xs[u], ys[u], zs[u], base + j + u);
      }
      for (; j < nj; ++j) test(qx[j], qy[j], qz[j], base + j);
   }
}
