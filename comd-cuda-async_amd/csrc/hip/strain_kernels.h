// strain_kernels.h -- the per-atom strain tensor and the non-affine displacement D^2min for gfx950 (comdStrainReferenceGpu, computeAtomStrain,
// computeAtomStrainSummary, comd_hip.h).  The reference has no counterpart.
//
// State: the reference table, one 32-byte record {x, y, z, spare} of doubles (in both precision builds) per GLOBAL atom id, the same on every rank:
// the position x0[g] of atom g when the reference was taken, and the box L0 of that moment.  StrainReference_Store writes the records of this rank's
// local atoms with plain vector stores (one thread owns a gid); the host adds the ranks' tables and uploads the sum.
//
// For every local atom i, with the neighbours j (local or halo image) at 0 < |d|^2 <= rs^2 in the CURRENT configuration, d = x_j - x_i formed in
// real_t (the halo positions carry their periodic shift) and d0 = x0[gid_j] - x0[gid_i] reduced per axis, in double, to the image of L0 nearest the current
// separation mapped back to the reference box, d0 -= L0 rint((d0 - d L0 / L) / L0) with L the current global box.  That is the image the pair was accepted
// through.  The shortest image, rint(d0 / L0), is the same one unless |d0| can pass L0 / 2 on an axis: a 2-cell axis with rs near the force cutoff, where it
// returns the other image and d0 is wrong by a whole box length.
//   V = sum d0 d0^T (6)   A = sum d d0^T (9)   S = sum |d|^2   n = the neighbours           -- 17 sums, in double in both builds
//   F = A V^-1 (the adjugate of the symmetric V over its determinant), so that d ~ F d0
//   E = 1/2 (F^T F - I)                the Green-Lagrange strain, xx yy zz yz xz xy
//   D^2 = max(0, S - F:A)              = sum_j |d - F d0|^2, the one-pass form of Falk and Langer's D^2min, not divided by n
// An atom with n < 3 or det V <= 1e-9 (tr V / 3)^3 is invalid: E and D^2 are NaN, n is still stored.
//
// Mapping: the chunk walk of stencil_walk.h, lane = atom i.  For an accepted j the kernel loads gid[j] and the record of that gid: in a full chunk j is
// wave-uniform and so are both loads.  A replicated chunk (reps > 1) has the atom's neighbours split among reps lanes `span` apart: their sums are added
// by a butterfly over the copies (ds_bpermute, s = span, 2 span, ... 32, a double as two dwords; a + b is what both lanes of a pair compute, so every
// copy ends with the same bits, in an order that depends on reps alone).  Copy 0 solves and stores.
// Output: seven SoA planes [7][nLocalBoxes*cap] of real_t (E six, D^2) and one plane of int (n).  No atomics, no LDS, no scratch; bit-reproducible.
// The kernel reads r, gid, the reference table and the cell tables and writes nothing but its planes.
//
// AtomStrain_Summary / AtomStrain_SummaryFinal: from the planes of the occupied slots, formed in double:
//   gamma_i = sqrt( E_yz^2 + E_xz^2 + E_xy^2 + [(E_xx - E_yy)^2 + (E_yy - E_zz)^2 + (E_zz - E_xx)^2] / 6 )       the shear invariant
//   vol_i   = (E_xx + E_yy + E_zz) / 3                                                                           the volumetric strain
// and sum gamma, max gamma with the gid that holds it (ties: the lowest gid), sum vol, sum D^2, max D^2, the atoms with gamma >= the threshold, the
// valid and the invalid atoms (a NaN in the E_xx plane; they stay out of sums and extremes).  A fixed grid walks the slots with a fixed stride, the
// workgroup combines in a fixed order and writes one row; the second stage combines the rows in a fixed order.
#pragma once
#include "stencil_walk.h"
#include "slot_summary.h"

#define ATOMSTRAIN_BLOCKS 2048         // the grid of the walk, as ATOMSTRESS_BLOCKS
#define ATOMSTRAIN_SUM_BLOCKS 512      // rows of the summary: fixed, so the order of the sums does not depend on the system
#define ATOMSTRAIN_SUM_N 9             // sum gamma, max gamma, its gid, sum vol, sum D^2, max D^2, valid atoms, invalid atoms, atoms at or above the threshold
#define ATOMSTRAIN_PLANES 7            // E xx yy zz yz xz xy, D^2

// the records of this rank's local atoms; the table was zeroed before
__global__ __launch_bounds__(256)
void StrainReference_Store(const real_t* __restrict__ rx, const real_t* __restrict__ ry, const real_t* __restrict__ rz, const int* __restrict__ nAtoms,
                           const int* __restrict__ gid, int cap, size_t nSlots, int nRef, double* __restrict__ ref)
{
   for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < nSlots; o += (size_t)gridDim.x * blockDim.x) {
      const size_t b = o / (size_t)cap;
      if ((int)(o - b * (size_t)cap) >= nAtoms[b]) continue;
      const int g = gid[o];
      if ((unsigned)g >= (unsigned)nRef) continue;
      double* __restrict__ rec = ref + 4 * (size_t)g;
      rec[0] = (double)rx[o]; rec[1] = (double)ry[o]; rec[2] = (double)rz[o]; rec[3] = 0.0;
   }
}

struct AtomStrainArgs : StencilArgs {
   const int* __restrict__ gid;
   const double* __restrict__ ref;     // [nRef][4]
   int nRef;
   real_t rs2;
   double L0x, L0y, L0z;
   double sx, sy, sz;                  // L0 / L per axis, L the current global box: a current separation mapped back to the reference box
   size_t plane;                       // nLocalBoxes * cap: the slots of one plane of the output
};

// out: [7][plane], outN: [plane].  Kernel parameters of their own, __restrict__, and not members of the argument record: see AtomStress_thread_atom
// (stress_kernels.h), which stores inside the loop over the chunks as this kernel does.
__global__ __launch_bounds__(256)
void AtomStrain_thread_atom(AtomStrainArgs v, real_t* __restrict__ out, int* __restrict__ outN)
{
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;

   forEachChunk(v, lane, wave, [&](int iBox, int first, int, int reps, int span, int q, int ia, bool active) {
      const size_t iOff = (size_t)iBox * v.cap + (active ? ia : first);
      const real_t xi = v.rx[iOff], yi = v.ry[iOff], zi = v.rz[iOff];
      const int gi = v.gid[iOff];
      const bool known = active && (unsigned)gi < (unsigned)v.nRef;
      const double* __restrict__ ri = v.ref + 4 * (size_t)(known ? gi : 0);
      const double x0i = ri[0], y0i = ri[1], z0i = ri[2];
      double vxx = 0.0, vyy = 0.0, vzz = 0.0, vyz = 0.0, vxz = 0.0, vxy = 0.0;
      double axx = 0.0, axy = 0.0, axz = 0.0, ayx = 0.0, ayy = 0.0, ayz = 0.0, azx = 0.0, azy = 0.0, azz = 0.0;      // A_ab = sum d_a d0_b
      double ss = 0.0;
      int n = 0;
      auto test = [&](real_t xj, real_t yj, real_t zj, size_t jOff) {
         const real_t ex = xj - xi, ey = yj - yi, ez = zj - zi;
         const real_t r2 = ex*ex + ey*ey + ez*ez;
         if (known && r2 <= v.rs2 && r2 > R(0.0)) {
            const int gj = v.gid[jOff];
            if ((unsigned)gj < (unsigned)v.nRef) {
               const double* __restrict__ rj = v.ref + 4 * (size_t)gj;
               double px = rj[0] - x0i, py = rj[1] - y0i, pz = rj[2] - z0i;
               const double dx = (double)ex, dy = (double)ey, dz = (double)ez;
               // the image of d0 nearest d mapped back to the reference box: the image the pair was accepted through, not the shortest one
               px -= v.L0x * __builtin_rint((px - dx * v.sx) / v.L0x); py -= v.L0y * __builtin_rint((py - dy * v.sy) / v.L0y);
               pz -= v.L0z * __builtin_rint((pz - dz * v.sz) / v.L0z);
               vxx = __builtin_fma(px, px, vxx); vyy = __builtin_fma(py, py, vyy); vzz = __builtin_fma(pz, pz, vzz);
               vyz = __builtin_fma(py, pz, vyz); vxz = __builtin_fma(px, pz, vxz); vxy = __builtin_fma(px, py, vxy);
               axx = __builtin_fma(dx, px, axx); axy = __builtin_fma(dx, py, axy); axz = __builtin_fma(dx, pz, axz);
               ayx = __builtin_fma(dy, px, ayx); ayy = __builtin_fma(dy, py, ayy); ayz = __builtin_fma(dy, pz, ayz);
               azx = __builtin_fma(dz, px, azx); azy = __builtin_fma(dz, py, azy); azz = __builtin_fma(dz, pz, azz);
               ss += (dx * dx + dy * dy) + dz * dz;
               n += 1;
            }
         }
      };
      stencilWalk<size_t>(v, iBox, reps, q, test);
      if (reps > 1) sumOverCopies(lane, span, vxx, vyy, vzz, vyz, vxz, vxy, axx, axy, axz, ayx, ayy, ayz, azx, azy, azz, ss, n);
      if (active && q == 0) {
         // the adjugate of V and its determinant
         const double c00 = vyy * vzz - vyz * vyz, c01 = vxz * vyz - vxy * vzz, c02 = vxy * vyz - vxz * vyy;
         const double c11 = vxx * vzz - vxz * vxz, c12 = vxy * vxz - vxx * vyz, c22 = vxx * vyy - vxy * vxy;
         const double det = (vxx * c00 + vxy * c01) + vxz * c02;
         const double t = ((vxx + vyy) + vzz) / 3.0;
         const bool valid = n >= 3 && det > 1e-9 * ((t * t) * t);
         const double inv = 1.0 / (valid ? det : 1.0);
         const double fxx = ((axx * c00 + axy * c01) + axz * c02) * inv, fxy = ((axx * c01 + axy * c11) + axz * c12) * inv, fxz = ((axx * c02 + axy * c12) + axz * c22) * inv;
         const double fyx = ((ayx * c00 + ayy * c01) + ayz * c02) * inv, fyy = ((ayx * c01 + ayy * c11) + ayz * c12) * inv, fyz = ((ayx * c02 + ayy * c12) + ayz * c22) * inv;
         const double fzx = ((azx * c00 + azy * c01) + azz * c02) * inv, fzy = ((azx * c01 + azy * c11) + azz * c12) * inv, fzz = ((azx * c02 + azy * c12) + azz * c22) * inv;
         const double nan = __builtin_nan("");
         double e[ATOMSTRAIN_PLANES];
         e[0] = 0.5 * (((fxx * fxx + fyx * fyx) + fzx * fzx) - 1.0);
         e[1] = 0.5 * (((fxy * fxy + fyy * fyy) + fzy * fzy) - 1.0);
         e[2] = 0.5 * (((fxz * fxz + fyz * fyz) + fzz * fzz) - 1.0);
         e[3] = 0.5 * ((fxy * fxz + fyy * fyz) + fzy * fzz);
         e[4] = 0.5 * ((fxx * fxz + fyx * fyz) + fzx * fzz);
         e[5] = 0.5 * ((fxx * fxy + fyx * fyy) + fzx * fzy);
         const double fa = (((fxx * axx + fxy * axy) + fxz * axz) + ((fyx * ayx + fyy * ayy) + fyz * ayz)) + ((fzx * azx + fzy * azy) + fzz * azz);
         const double d2 = ss - fa;
         e[6] = d2 > 0.0 ? d2 : 0.0;
         real_t* __restrict__ o = out + iOff;
#pragma unroll
         for (int c = 0; c < ATOMSTRAIN_PLANES; ++c) o[(size_t)c * v.plane] = (real_t)(valid ? e[c] : nan);
         outN[iOff] = n;
      }
   });
}

// one candidate of the summary (slot_summary.h): the sums and the counts add, the extremes compare; of two equal gamma the lower gid stays
struct AtomStrainSum {
   double sumG, maxG, sumV, sumD, maxD;
   int gid, n, bad, above;
   static constexpr int N = ATOMSTRAIN_SUM_N;

   __device__ static AtomStrainSum empty() { return AtomStrainSum{ 0.0, -__builtin_huge_val(), 0.0, 0.0, -__builtin_huge_val(), -1, 0, 0, 0 }; }
   __device__ void join(const AtomStrainSum& b)
   {
      sumG += b.sumG; sumV += b.sumV; sumD += b.sumD; n += b.n; bad += b.bad; above += b.above;
      maxD = b.maxD > maxD ? b.maxD : maxD;
      const bool take = b.gid >= 0 && (gid < 0 || b.maxG > maxG || (b.maxG == maxG && b.gid < gid));
      maxG = take ? b.maxG : maxG; gid = take ? b.gid : gid;
   }
   __device__ void toRow(double* __restrict__ row) const
   {
      row[0] = sumG; row[1] = maxG; row[2] = (double)gid; row[3] = sumV; row[4] = sumD; row[5] = maxD;
      row[6] = (double)n; row[7] = (double)bad; row[8] = (double)above;
   }
   __device__ static AtomStrainSum fromRow(const double* __restrict__ row)
   {
      return AtomStrainSum{ row[0], row[1], row[3], row[4], row[5], (int)row[2], (int)row[6], (int)row[7], (int)row[8] };
   }
};

// stage 1: gamma, vol and D^2 of the occupied slots of the planes; an invalid atom counts and stays out of the rest
__global__ __launch_bounds__(256)
void AtomStrain_Summary(const real_t* __restrict__ planes, size_t plane, const int* __restrict__ nAtoms, const int* __restrict__ gid, int cap,
                        double threshold, double* __restrict__ partial)
{
   summaryOfSlots<AtomStrainSum>(plane, nAtoms, cap, partial, [&](size_t o) {
      const double xx = (double)planes[o], yy = (double)planes[plane + o], zz = (double)planes[2 * plane + o];
      const double yz = (double)planes[3 * plane + o], xz = (double)planes[4 * plane + o], xy = (double)planes[5 * plane + o];
      const double d2 = (double)planes[6 * plane + o];
      AtomStrainSum c = AtomStrainSum::empty();
      if (xx != xx) c.bad = 1;
      else {
         const double d0 = xx - yy, d1 = yy - zz, d2e = zz - xx;
         const double g = __builtin_sqrt(((yz * yz + xz * xz) + xy * xy) + ((d0 * d0 + d1 * d1) + d2e * d2e) / 6.0);
         c.sumG = g; c.maxG = g; c.sumV = ((xx + yy) + zz) / 3.0; c.sumD = d2; c.maxD = d2; c.gid = gid[o]; c.n = 1; c.above = g >= threshold ? 1 : 0;
      }
      return c;
   });
}

// stage 2: the rows -> out[ATOMSTRAIN_SUM_N]
__global__ __launch_bounds__(256)
void AtomStrain_SummaryFinal(const double* __restrict__ partial, int nPartial, double* __restrict__ out)
{
   summaryOfRows<AtomStrainSum>(partial, nPartial, out);
}
