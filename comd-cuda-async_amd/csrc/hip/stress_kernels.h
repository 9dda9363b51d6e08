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
#include "slot_summary.h"

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
      if (reps > 1) sumOverCopies(lane, span, wxx, wyy, wzz, wyz, wxz, wxy);
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

// one candidate of the summary (slot_summary.h): the two sums and the count add, the extremes compare; of two equal sigma the lower gid stays
struct AtomStressSum {
   double sumP, minP, maxP, sumS, maxS;
   int gid, n;
   static constexpr int N = ATOMSTRESS_SUM_N;

   __device__ static AtomStressSum empty() { return AtomStressSum{ 0.0, __builtin_huge_val(), -__builtin_huge_val(), 0.0, -__builtin_huge_val(), -1, 0 }; }
   __device__ void join(const AtomStressSum& b)
   {
      sumP += b.sumP; sumS += b.sumS; n += b.n;
      minP = b.minP < minP ? b.minP : minP;
      maxP = b.maxP > maxP ? b.maxP : maxP;
      const bool take = b.gid >= 0 && (gid < 0 || b.maxS > maxS || (b.maxS == maxS && b.gid < gid));
      maxS = take ? b.maxS : maxS; gid = take ? b.gid : gid;
   }
   __device__ void toRow(double* __restrict__ row) const
   {
      row[0] = sumP; row[1] = minP; row[2] = maxP; row[3] = sumS; row[4] = maxS; row[5] = (double)gid; row[6] = (double)n;
   }
   __device__ static AtomStressSum fromRow(const double* __restrict__ row) { return AtomStressSum{ row[0], row[1], row[2], row[3], row[4], (int)row[5], (int)row[6] }; }
};

// stage 1: p and sigma of the occupied slots of the planes
__global__ __launch_bounds__(256)
void AtomStress_Summary(const real_t* __restrict__ planes, size_t plane, const int* __restrict__ nAtoms, const int* __restrict__ gid, int cap,
                        double invOmega, double* __restrict__ partial)
{
   const double third = invOmega / 3.0;
   summaryOfSlots<AtomStressSum>(plane, nAtoms, cap, partial, [&](size_t o) {
      const double xx = (double)planes[o], yy = (double)planes[plane + o], zz = (double)planes[2 * plane + o];
      const double yz = (double)planes[3 * plane + o], xz = (double)planes[4 * plane + o], xy = (double)planes[5 * plane + o];
      const double p = -((xx + yy) + zz) * third;
      const double d0 = xx - yy, d1 = yy - zz, d2 = zz - xx;
      const double s = __builtin_sqrt(0.5 * ((d0 * d0 + d1 * d1) + d2 * d2) + 3.0 * ((yz * yz + xz * xz) + xy * xy)) * invOmega;
      return AtomStressSum{ p, p, p, s, s, gid[o], 1 };
   });
}

// stage 2: the rows -> out[ATOMSTRESS_SUM_N]
__global__ __launch_bounds__(256)
void AtomStress_SummaryFinal(const double* __restrict__ partial, int nPartial, double* __restrict__ out)
{
   summaryOfRows<AtomStressSum>(partial, nPartial, out);
}
