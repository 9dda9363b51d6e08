// stress_kernels.h -- the per-atom virial stress for gfx950 (computeAtomStress, computeAtomStressSummary, comd_hip.h).  The reference has no counterpart.
//
// For every local atom i, six components in the order xx yy zz yz xz xy, in eV (stress x volume, tension positive):
//   s_i,ab = -( [kinetic] p_i,a p_i,b / m_i  +  1/2 sum_j r_ij,a f_ij,b )
// j over the neighbours (local or halo image) with 0 < |r_ij|^2 <= rc^2, r_ij = r_i - r_j, f_ij the force on i due to j: the pair convention of
// virial_kernels.h -- its acceptance test, its functors (VirialLj, VirialLjTable, VirialEam<SPLINE>; EAM reads F'_j from dfEmbed, halo slots
// included), each pair weighing 1/2 on either side -- so that sum_i s_i = -(K + W) of computeVirial on the same state.
//
// Mapping: the chunk walk of stencil_walk.h, lane = atom i; each lane keeps its six sums in real_t, as Virial_thread_atom does, but instead of
// adding them over the atoms it stores them.  A replicated chunk (reps > 1) has the atom's neighbours split among reps lanes `span` apart: their
// partial sums are added by a butterfly over the copies (ds_bpermute, s = span, 2 span, ... 32; a + b is what both lanes of a pair compute, so
// every copy ends with the same bits, in an order that depends on reps alone).  Copy 0 then adds the kinetic term when asked and stores.
// Output: six SoA planes [6][nLocalBoxes*cap] of real_t: consecutive lanes store consecutive slots of a plane.  No atomics, no LDS, no scratch;
// bit-reproducible.  The kernel reads r, p, dfEmbed and the cell tables and writes nothing but its planes.
//
// AtomStress_Summary / AtomStress_SummaryFinal: from the planes of the occupied slots, formed in double with the uniform atomic volume omega:
//   p_i     = -(s_xx + s_yy + s_zz) / (3 omega)                                                              hydrostatic pressure
//   sigma_i = sqrt( 1/2 [(s_xx - s_yy)^2 + (s_yy - s_zz)^2 + (s_zz - s_xx)^2] + 3 (s_yz^2 + s_xz^2 + s_xy^2) ) / omega    von Mises stress
// and sum p, min p, max p, sum sigma, max sigma with the gid that holds it (ties: the lowest gid), and the number of atoms.  A fixed grid walks
// the slots with a fixed stride, the workgroup combines in a fixed order and writes one row; the second stage combines the rows in a fixed order.
#pragma once
#include "virial_kernels.h"

#define ATOMSTRESS_BLOCKS 2048         // the grid of the walk, as VIRIAL_BLOCKS
#define ATOMSTRESS_SUM_BLOCKS 512      // rows of the summary: fixed, so the order of the sums does not depend on the system
#define ATOMSTRESS_SUM_N 7             // sum p, min p, max p, sum sigma, max sigma, its gid, atoms

struct AtomStressArgs : StencilArgs {
   const real_t* __restrict__ px; const real_t* __restrict__ py; const real_t* __restrict__ pz;
   const int* __restrict__ iSpecies; const real_t* __restrict__ speciesMass;
   real_t rc2;
   int withKinetic;
   size_t plane;                       // nLocalBoxes * cap: the slots of one plane of the output
};

// out: [6][plane].  It is a kernel parameter of its own, __restrict__, and not a member of the argument record: this kernel stores inside the loop over the
// chunks, and only the noalias of a parameter lets the compiler prove that the stores leave r, dfEmbed and the cell tables alone.  As a member it gave up the
// scalar-load stream of the full chunks for per-lane loads: 84 VGPRs instead of 51 (analytic LJ, double build) and 9.1 ms instead of the virial's 7.2 at 80^3.
template <class PAIR>
__global__ __launch_bounds__(256)
void AtomStress_thread_atom(AtomStressArgs v, PAIR pair, real_t* __restrict__ out)
{
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;

   forEachChunk(v, lane, wave, [&](int iBox, int first, int, int reps, int span, int q, int ia, bool active) {
      const size_t iOff = (size_t)iBox * v.cap + (active ? ia : first);
      const real_t xi = v.rx[iOff], yi = v.ry[iOff], zi = v.rz[iOff];
      pair.begin(iOff);
      real_t wxx = R(0.0), wyy = R(0.0), wzz = R(0.0), wyz = R(0.0), wxz = R(0.0), wxy = R(0.0);
      auto test = [&](real_t xj, real_t yj, real_t zj, size_t jOff) {
         const real_t dx = xi - xj, dy = yi - yj, dz = zi - zj;
         const real_t r2 = dx*dx + dy*dy + dz*dz;
         if (active && r2 <= v.rc2 && r2 > R(0.0)) {
            real_t gx = R(0.0), gy = R(0.0), gz = R(0.0);
            pair(dx, dy, dz, r2, jOff, gx, gy, gz);
            wxx = fmaR(dx, gx, wxx); wyy = fmaR(dy, gy, wyy); wzz = fmaR(dz, gz, wzz);
            wyz = fmaR(dy, gz, wyz); wxz = fmaR(dx, gz, wxz); wxy = fmaR(dx, gy, wxy);
         }
      };
      stencilWalk<size_t>(v, iBox, reps, q, test);
      if (reps > 1) {
         // the copies' shares into one: after the doubling over s every lane holds the sum over the copies lane ^ s, lane ^ 2s, ... as well
         for (int s = span; s < WAVE; s <<= 1) {
            const int addr = (lane ^ s) << 2;
            wxx += bpermuteAddrR(wxx, addr); wyy += bpermuteAddrR(wyy, addr); wzz += bpermuteAddrR(wzz, addr);
            wyz += bpermuteAddrR(wyz, addr); wxz += bpermuteAddrR(wxz, addr); wxy += bpermuteAddrR(wxy, addr);
         }
      }
      if (active && q == 0) {
         const real_t h = R(0.5) * pair.scale();
         real_t kxx = R(0.0), kyy = R(0.0), kzz = R(0.0), kyz = R(0.0), kxz = R(0.0), kxy = R(0.0);
         if (v.withKinetic) {
            const real_t invMass = R(1.0) / v.speciesMass[v.iSpecies[iOff]];
            const real_t qx = v.px[iOff], qy = v.py[iOff], qz = v.pz[iOff];
            kxx = (qx * qx) * invMass; kyy = (qy * qy) * invMass; kzz = (qz * qz) * invMass;
            kyz = (qy * qz) * invMass; kxz = (qx * qz) * invMass; kxy = (qx * qy) * invMass;
         }
         real_t* __restrict__ o = out + iOff;
         o[0]           = -fmaR(h, wxx, kxx); o[v.plane]     = -fmaR(h, wyy, kyy); o[2 * v.plane] = -fmaR(h, wzz, kzz);
         o[3 * v.plane] = -fmaR(h, wyz, kyz); o[4 * v.plane] = -fmaR(h, wxz, kxz); o[5 * v.plane] = -fmaR(h, wxy, kxy);
      }
   });
}

// one candidate of the summary: the two sums and the count add, the extremes compare; of two equal sigma the lower gid stays
struct AtomStressSum {
   double sumP, minP, maxP, sumS, maxS;
   int gid, n;
};

__device__ __forceinline__ void atomStressJoin(AtomStressSum& a, const AtomStressSum& b)
{
   a.sumP += b.sumP; a.sumS += b.sumS; a.n += b.n;
   a.minP = b.minP < a.minP ? b.minP : a.minP;
   a.maxP = b.maxP > a.maxP ? b.maxP : a.maxP;
   const bool take = b.gid >= 0 && (a.gid < 0 || b.maxS > a.maxS || (b.maxS == a.maxS && b.gid < a.gid));
   a.maxS = take ? b.maxS : a.maxS; a.gid = take ? b.gid : a.gid;
}

// over the 64 lanes, then over the 4 waves, in a fixed order; thread 0 ends with the workgroup's candidate
__device__ __forceinline__ void atomStressBlockJoin(AtomStressSum& a, double (*sD)[5], int (*sI)[2])
{
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;
#pragma unroll
   for (int m = 32; m >= 1; m >>= 1) {
      const int src = lane ^ m;
      AtomStressSum b;
      b.sumP = bpermuteR(a.sumP, src); b.minP = bpermuteR(a.minP, src); b.maxP = bpermuteR(a.maxP, src);
      b.sumS = bpermuteR(a.sumS, src); b.maxS = bpermuteR(a.maxS, src);
      b.gid = __builtin_amdgcn_ds_bpermute(src << 2, a.gid); b.n = __builtin_amdgcn_ds_bpermute(src << 2, a.n);
      atomStressJoin(a, b);      // symmetric in its operands (a + b, the extremes, the lower gid): both lanes of a pair end with the same bits
   }
   if (lane == 0) { sD[wave][0] = a.sumP; sD[wave][1] = a.minP; sD[wave][2] = a.maxP; sD[wave][3] = a.sumS; sD[wave][4] = a.maxS; sI[wave][0] = a.gid; sI[wave][1] = a.n; }
   __syncthreads();
   if (threadIdx.x == 0) {
      for (int w = 1; w < 4; ++w) {
         AtomStressSum b;
         b.sumP = sD[w][0]; b.minP = sD[w][1]; b.maxP = sD[w][2]; b.sumS = sD[w][3]; b.maxS = sD[w][4]; b.gid = sI[w][0]; b.n = sI[w][1];
         atomStressJoin(a, b);
      }
   }
}

__device__ __forceinline__ AtomStressSum atomStressEmpty()
{
   AtomStressSum a;
   a.sumP = 0.0; a.minP = __builtin_huge_val(); a.maxP = -__builtin_huge_val(); a.sumS = 0.0; a.maxS = -__builtin_huge_val();
   a.gid = -1; a.n = 0;
   return a;
}

// stage 1: the occupied slots of the planes -> one row per workgroup, partial[blockIdx.x][ATOMSTRESS_SUM_N] (gid and count as doubles: exact)
__global__ __launch_bounds__(256)
void AtomStress_Summary(const real_t* __restrict__ planes, size_t plane, const int* __restrict__ nAtoms, const int* __restrict__ gid, int cap,
                        double invOmega, double* __restrict__ partial)
{
   __shared__ double sD[4][5];
   __shared__ int sI[4][2];
   AtomStressSum a = atomStressEmpty();
   const double third = invOmega / 3.0;
   for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < plane; o += (size_t)gridDim.x * blockDim.x) {
      const size_t b = o / (size_t)cap;
      if ((int)(o - b * (size_t)cap) >= nAtoms[b]) continue;
      const double xx = (double)planes[o], yy = (double)planes[plane + o], zz = (double)planes[2 * plane + o];
      const double yz = (double)planes[3 * plane + o], xz = (double)planes[4 * plane + o], xy = (double)planes[5 * plane + o];
      const double p = -((xx + yy) + zz) * third;
      const double d0 = xx - yy, d1 = yy - zz, d2 = zz - xx;
      const double s = __builtin_sqrt(0.5 * ((d0 * d0 + d1 * d1) + d2 * d2) + 3.0 * ((yz * yz + xz * xz) + xy * xy)) * invOmega;
      AtomStressSum c;
      c.sumP = p; c.minP = p; c.maxP = p; c.sumS = s; c.maxS = s; c.gid = gid[o]; c.n = 1;
      atomStressJoin(a, c);
   }
   atomStressBlockJoin(a, sD, sI);
   if (threadIdx.x == 0) {
      double* row = partial + (size_t)blockIdx.x * ATOMSTRESS_SUM_N;
      row[0] = a.sumP; row[1] = a.minP; row[2] = a.maxP; row[3] = a.sumS; row[4] = a.maxS; row[5] = (double)a.gid; row[6] = (double)a.n;
   }
}

// stage 2: the rows -> out[ATOMSTRESS_SUM_N], in a fixed order
__global__ __launch_bounds__(256)
void AtomStress_SummaryFinal(const double* __restrict__ partial, int nPartial, double* __restrict__ out)
{
   __shared__ double sD[4][5];
   __shared__ int sI[4][2];
   AtomStressSum a = atomStressEmpty();
   for (int i = threadIdx.x; i < nPartial; i += blockDim.x) {
      const double* row = partial + (size_t)i * ATOMSTRESS_SUM_N;
      AtomStressSum c;
      c.sumP = row[0]; c.minP = row[1]; c.maxP = row[2]; c.sumS = row[3]; c.maxS = row[4]; c.gid = (int)row[5]; c.n = (int)row[6];
      atomStressJoin(a, c);
   }
   atomStressBlockJoin(a, sD, sI);
   if (threadIdx.x == 0) {
      out[0] = a.sumP; out[1] = a.minP; out[2] = a.maxP; out[3] = a.sumS; out[4] = a.maxS; out[5] = (double)a.gid; out[6] = (double)a.n;
   }
}
