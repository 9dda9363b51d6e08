// csp_kernels.h -- per-atom defect analysis for gfx950: the centro-symmetry parameter and the coordination number (computeCentroSymmetry,
// comd_hip.h).  The reference has no counterpart.
//
// For every local atom i, with the neighbours j != i (local or halo image) at |r_j - r_i| < the force cutoff:
//   coord_i = number of neighbours with |r_ij| < rCoord                                  (rCoord <= cutoff, the host checks)
//   csp_i   = sum of the 6 smallest of the 66 values |R_a + R_b|^2, a < b, added in ascending order, R_1..R_12 = r_j - r_i of the 12 nearest
//             neighbours (Kelchner, Plimpton, Hamilton 1998); +inf for an atom with fewer than 12 neighbours inside the cutoff.
// A tie between the 12th and the 13th nearest distance goes to the neighbour met first in walk order (stencil cell by stencil cell, slot by
// slot; with a replicated chunk, see below, the copy with the lower number wins).
//
// Mapping: the chunk walk of stencil_walk.h, which also says why 27 cells are enough for the cells of the *_nl methods and of -L.
//
// The 12 nearest: every lane keeps {r^2, slot} of its 12 best candidates sorted by r^2 in registers.  A candidate closer than the lane's 12th
// (which starts at cutoff^2, so this is the cutoff test too) is carried through the 12 positions with compare / select at compile-time indices: it
// settles where it belongs and pushes the rest down, the last one out.  No array is indexed at run time, so nothing goes to scratch.  The
// chain runs only when some lane of the wave takes a candidate; a lane's threshold falls quickly, so most candidates are refused by the one compare.
// Slots are kept, not offset vectors (12 VGPRs instead of 72 in the double build): the positions are read again at the end.  The halo
// cells hold shifted images, so r_j - r_i is the offset vector as it stands, without a minimum image.
//
// Small chunks: a chunk of at most 32 atoms -- every EAM cell, LJ at 2.5 sigma, the tail chunk of an LJ cell -- would use 10 to 50 % of the lanes.  It
// is replicated (stencil_walk.h): reps copies of its atoms, copy q walks the stencil cells q, q + reps, ... with per-lane loads, and the
// partial sets are merged by a butterfly over the copies (each lane reads the 12 entries of the lane `span` away through ds_bpermute and offers
// them to its own set; the coordination counts add).  Packing several cells into a wave instead would keep the loads scalar only for the lanes of one
// cell at a time and needs a per-lane cell table; replication reuses the walk the histogram and the virial already have, and the merge costs
// 12 offers per doubling against the 27 / reps cells of candidates it saves.  The 66-pair stage at the end is NOT shared among the copies: only copy 0
// keeps its result, so on an EAM cell it runs on about 14 of 64 lanes.  The reason: a lane that took a share of the 66 pairs of its own would index
// X[a], X[b] at run time (scratch), and predicating shares on compile-time indices leaves every lane issuing all 66 anyway.  Measured at 80^3 the EAM
// kernel takes 4.3 ms against 10.2 ms for LJ 5 sigma: this stage and the merge are what does not shrink with the candidates.
//
// The selection and the merge are the text of nearest12_walk.h, which Cna_thread_atom (cna_kernels.h) includes too; the 66-pair stage is this kernel's own.
//
// The kernel reads r, nAtoms and nbr and writes nothing but its own two per-slot buffers; no atomics: bit-reproducible.
#pragma once
#include "stencil_walk.h"

#define CSP_BLOCKS 2048
#define CSP_NN 12                      // neighbours of the parameter: the first FCC shell

struct CentroSymArgs : StencilArgs {
   real_t rc2, rCoord2;               // cutoff^2, rCoord^2
   real_t* __restrict__ csp;           // [nLocalBoxes*cap]
   int* __restrict__ coord;            // [nLocalBoxes*cap]
};

// offer {c, ci} to the ascending set: it settles at its place, what was there moves on, the last one drops out.  On equal keys the entry that is in stays.
template <int N>
__device__ __forceinline__ void cspOffer(real_t (&d)[N], int (&id)[N], real_t c, int ci)
{
#pragma unroll
   for (int k = 0; k < N; ++k) {
      const bool lt = c < d[k];
      const real_t lo = lt ? c : d[k], hi = lt ? d[k] : c;
      const int loI = lt ? ci : id[k], hiI = lt ? id[k] : ci;
      d[k] = lo; id[k] = loI; c = hi; ci = hiI;
   }
}

// the same for keys alone
template <int N>
__device__ __forceinline__ void cspOfferKey(real_t (&d)[N], real_t c)
{
#pragma unroll
   for (int k = 0; k < N; ++k) {
      const bool lt = c < d[k];
      const real_t lo = lt ? c : d[k], hi = lt ? d[k] : c;
      d[k] = lo; c = hi;
   }
}

__global__ __launch_bounds__(256, 4)
void CentroSym_thread_atom(CentroSymArgs v)
{
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;
   const real_t inf = R(__builtin_huge_val());

   forEachChunk(v, lane, wave, [&](int iBox, int first, int, int reps, int span, int q, int ia, bool active) {
#define NN12_COORD(x) x
#include "nearest12_walk.h"       // the 12 nearest of the lane's atom: me, xi, yi, zi, d[], id[], coord
#undef NN12_COORD

      if (active && q == 0) {
         const bool full = id[CSP_NN - 1] >= 0;
         real_t X[CSP_NN], Y[CSP_NN], Z[CSP_NN];
#pragma unroll
         for (int k = 0; k < CSP_NN; ++k) {
            const int s = full ? id[k] : me;
            X[k] = v.rx[s] - xi; Y[k] = v.ry[s] - yi; Z[k] = v.rz[s] - zi;
         }
         real_t t[6];
#pragma unroll
         for (int k = 0; k < 6; ++k) t[k] = inf;
#pragma unroll
         for (int a = 0; a < CSP_NN; ++a)
#pragma unroll
            for (int b = a + 1; b < CSP_NN; ++b) {
               const real_t sx = X[a] + X[b], sy = Y[a] + Y[b], sz = Z[a] + Z[b];
               cspOfferKey<6>(t, sx*sx + sy*sy + sz*sz);
            }
         const real_t sum = ((((t[0] + t[1]) + t[2]) + t[3]) + t[4]) + t[5];
         v.csp[me] = full ? sum : inf;
         v.coord[me] = coord;
      }
   });
}
