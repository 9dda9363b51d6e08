// cna_kernels.h -- per-atom structure identification for gfx950: adaptive common neighbour analysis (computeCommonNeighbors, comd_hip.h).  The
// reference has no counterpart.
//
// Adaptive CNA (Stukowski 2012, as in OVITO) restricted to the 12-neighbour signatures.  For every local atom i:
//   the set    its 12 nearest neighbours j != i (local or halo image) with |r_j - r_i| < the force cutoff, chosen exactly as CentroSym_thread_atom chooses
//              them (strict <, a tie goes to the neighbour met first in walk order); fewer than 12 inside the cutoff: CNA_OTHER;
//   r_loc      (1 + sqrt 2)/2 times the mean of the 12 distances, added in ascending order;
//   bonds      neighbours a != b are bonded when |R_a - R_b|^2 <= r_loc^2 (66 tests); the 12 bonds to the centre are taken as given;
//   signature  of neighbour a, with C_a = the neighbours bonded to a: n_cn = |C_a|, n_b = the bonds among the members of C_a, l_cb = the bonds of the
//              largest connected cluster of those;
//   type       CNA_FCC 1: twelve (4,2,1); CNA_HCP 2: six (4,2,1) and six (4,2,2); CNA_ICO 4: twelve (5,5,5); CNA_OTHER 0 for the rest.  3 is OVITO's BCC,
//              which needs 14 neighbours and a cutoff beyond the second shell: never returned.
//
// The mapping is the chunk walk of stencil_walk.h; the selection of the 12 and the butterfly merge of replicated chunks are nearest12_walk.h, the
// text CentroSym_thread_atom compiles too.  After it the lane reads the 12 offset vectors again (36 values, in ascending order of distance; the
// distances are computed from them, so the sorted keys die with the walk), and builds one 12-bit mask per neighbour from the 66 tests, all at
// compile-time indices; from there on the offsets are dead and the state is 12 integers.
//
// Registers (double build: 128 VGPRs, the 4 waves per SIMD of the csp kernel, no scratch; float: 115).  The walk alone fills the double build's budget, so
// the stage must add nothing that lives across it and nothing that overflows into VGPRs: see signBit, CNA_ROW_FENCE and the store at the end.
//
// l_cb without a graph search.  deg_a(b) = popcount(adj[b] & adj[a]) is the degree of b inside C_a, so n_b = half the sum over b in C_a, and
//   n_cn = 4, n_b = 2: the two bonds share an atom (l_cb = 2) exactly when some member has degree 2, otherwise they are apart (l_cb = 1);
//   n_cn = 5, n_b = 5, largest degree 2: the degrees add to 10, so every one is 2, and the only 2-regular graph on 5 nodes is one 5-ring (l_cb = 5).
// Every other (n_cn, n_b) makes the atom CNA_OTHER whatever l_cb is.  tests/test_cna.py computes l_cb by a connected-component search.
//
// Replicated chunks: after the merge every copy holds the same set, and only copy 0 runs the stage, as in the csp kernel.  Dealing the 12 signatures
// over the copies by predication on compile-time indices was not built: the copies of an atom are lanes of one wave, and a wave issues an
// instruction when any of its lanes wants it, so with the shares spread over the copies every signature is still issued once per wave, and the
// masks, which every share needs, are still built by all.  The instruction count of the wave cannot fall that way, only its EXEC occupancy rises.
//
// The kernel reads r, nAtoms and nbr and writes one int per slot; no atomics, integer output: bit-reproducible.
#pragma once
#include "csp_kernels.h"

#define CNA_BLOCKS 2048
#define CNA_OTHER 0
#define CNA_FCC 1
#define CNA_HCP 2
#define CNA_ICO 4

struct CnaArgs : StencilArgs {
   real_t rc2;                        // cutoff^2
   int* __restrict__ type;             // [nLocalBoxes*cap]
};

// 1 for x < 0, 0 for x >= 0 (+0 included): the sign bit, so that the 66 bond tests stay in the vector unit.  As compares (and the optimiser turns a plain
// shift of the sign back into one, hence the empty asm the value passes through) they are 66 lane masks, each alive until its second use, more scalar
// registers than a wave has; the overflow is parked in VGPRs, which the walk has none to spare of, and ends in scratch.
__device__ __forceinline__ unsigned signBit(double x) { unsigned s = (unsigned)__double2hiint(x) >> 31; asm("" : "+v"(s)); return s; }
__device__ __forceinline__ unsigned signBit(float x) { unsigned s = __float_as_uint(x) >> 31; asm("" : "+v"(s)); return s; }

// The 66 bond tests do not depend on one another, nor do the 12 signatures, and left alone the scheduler starts many at once.  A fence after each row of
// tests and each signature keeps what is in flight to one row: no instruction is moved across it.
#define CNA_ROW_FENCE() __builtin_amdgcn_sched_barrier(0)

__global__ __launch_bounds__(256, 4)
void Cna_thread_atom(CnaArgs v)
{
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;

   forEachChunk(v, lane, wave, [&](int iBox, int first, int, int reps, int span, int q, int ia, bool active) {
#define NN12_COORD(x)
#include "nearest12_walk.h"       // the 12 nearest of the lane's atom: me, xi, yi, zi, d[], id[]
#undef NN12_COORD

      if (active && q == 0) {
         const bool full = id[CSP_NN - 1] >= 0;
         real_t X[CSP_NN], Y[CSP_NN], Z[CSP_NN];
#pragma unroll
         for (int k = 0; k < CSP_NN; ++k) {
            const int s = id[k] > 0 ? id[k] : 0;              // an empty entry (-1) reads slot 0: the result is CNA_OTHER whatever comes of it
            X[k] = v.rx[s] - xi; Y[k] = v.ry[s] - yi; Z[k] = v.rz[s] - zi;
         }
         // r_loc^2: the 12 distances, computed again from the offsets (the sorted keys are not kept past the walk), added in ascending order
         real_t sum = R(0.0);
#pragma unroll
         for (int k = 0; k < CSP_NN; ++k) { const real_t r2 = X[k]*X[k] + Y[k]*Y[k] + Z[k]*Z[k]; sum += r2 * rsqrtR(r2); }
         const real_t rLoc = R(1.2071067811865475244) * (sum / R(12.0));
         const real_t rLoc2 = rLoc * rLoc;
         CNA_ROW_FENCE();
         unsigned apart[CSP_NN];                           // bit b of apart[a]: neighbours a and b are NOT bonded
#pragma unroll
         for (int k = 0; k < CSP_NN; ++k) apart[k] = 1u << k;
#pragma unroll
         for (int a = 0; a < CSP_NN; ++a)
#pragma unroll
            for (int b = 0; b < CSP_NN; ++b) {            // a constant trip count: the loop unrolls whole before a is known
               if (b <= a) continue;
               const real_t sx = X[a] - X[b], sy = Y[a] - Y[b], sz = Z[a] - Z[b];
               const unsigned far = signBit(rLoc2 - (sx*sx + sy*sy + sz*sz));
               apart[a] |= far << b;
               apart[b] |= far << a;
               if (b == CSP_NN - 1) CNA_ROW_FENCE();
            }
         unsigned adj[CSP_NN];
#pragma unroll
         for (int k = 0; k < CSP_NN; ++k) adj[k] = ~apart[k] & 0xfffu;
         int n421 = 0, n422 = 0, n555 = 0;
#pragma unroll
         for (int a = 0; a < CSP_NN; ++a) {
            const unsigned ca = adj[a];
            const int ncn = __builtin_popcount(ca);
            int degSum = 0, degMax = 0;
#pragma unroll
            for (int b = 0; b < CSP_NN; ++b) {
               if (b == a) continue;                       // a is not in C_a
               const int deg = __builtin_popcount(adj[b] & ca) & -(int)(ca >> b & 1u);
               degSum += deg;
               degMax = deg > degMax ? deg : degMax;
            }
            n421 += (ncn == 4 && degSum == 4 && degMax == 1) ? 1 : 0;
            n422 += (ncn == 4 && degSum == 4 && degMax == 2) ? 1 : 0;
            n555 += (ncn == 5 && degSum == 10 && degMax == 2) ? 1 : 0;
            CNA_ROW_FENCE();
         }
         int type = CNA_OTHER;
         if (n421 == 12) type = CNA_FCC;
         if (n421 == 6 && n422 == 6) type = CNA_HCP;
         if (n555 == 12) type = CNA_ICO;
         // the slot passes through an empty asm: otherwise its 64-bit form, made for the loads of xi, yi, zi, is kept for this store across the whole walk
         // next to the 32-bit one, the two registers the double build does not have (12 bytes of scratch)
         int out = me;
         asm("" : "+v"(out));
         v.type[out] = full ? type : CNA_OTHER;
      }
   });
}
