// virial_kernels.h -- the pair virial and the kinetic tensor for gfx950 (computeVirial, comd_hip.h).  The reference has no counterpart.
//
//   W_ab = sum_{i<j} r_ij,a f_ij,b     (r_ij = r_i - r_j to the image j interacts with, f_ij the force on i due to j)
//   K_ab = sum_i p_i,a p_i,b / m_i
// Components in the order xx yy zz yz xz xy.  Every instance evaluates the pair through the device helper of the force kernels of its
// mode -- ljPair, ljTablePair, interpolate<CLAMP> of phi and rho, interpolateSpline -- so the virial is the one of the forces that move the atoms:
//   LJ:  f_ij = ljPair's f_pair (x 24 eps s6 once per lane) or ljTablePair's -v'(r)/r d
//   EAM: f_ij = -(phi'(r) + (F'_i + F'_j) rho'(r)) / r d, F'_j read from dfEmbed, whose halo slots the force exchange has filled.
//
// Mapping: the chunk walk of stencil_walk.h, which also says why 27 cells are enough for the cells of the *_nl methods and of -L.  A full chunk
// reads F'_j through the scalar unit with the position of j.  Every pair is seen from both sides and weighs 1/2.
//
// Reduction: each lane accumulates its 6 + 6 components in real_t, the workgroup sums them in double in a fixed order and writes one row of 12
// partials; Virial_Final adds the rows in a fixed order (no atomics: runs are bit-reproducible).  The kernels read r, p, dfEmbed and the cell
// tables and write nothing but their partial rows.
#pragma once
#include "stencil_walk.h"
#include "lj_kernels.h"
#include "lj_table_kernels.h"
#include "eam_kernels.h"

#define VIRIAL_N 12                    // 6 virial + 6 kinetic components
#define VIRIAL_BLOCKS 2048             // rows of partials: fixed, so the order of the sums does not depend on the system

struct VirialArgs : StencilArgs {
   const real_t* __restrict__ px; const real_t* __restrict__ py; const real_t* __restrict__ pz;
   const int* __restrict__ iSpecies; const real_t* __restrict__ speciesMass;
   real_t rc2;
   double* __restrict__ partial;       // [gridDim.x][VIRIAL_N]
};

// The pair functors: begin(iOff) once per i atom, then operator() per accepted pair returns f_ij / scale in (gx, gy, gz).
struct VirialLj {
   LjArgs a;
   __host__ __device__ real_t scale() const { return LJ_FORCE_SCALE(a); }
   __device__ void begin(size_t) {}
   __device__ void operator()(real_t dx, real_t dy, real_t dz, real_t r2, size_t, real_t& gx, real_t& gy, real_t& gz) const
   {
      real_t e = R(0.0);
      ljPair<false>(dx, dy, dz, r2, a, gx, gy, gz, e);
   }
};

struct VirialLjTable {
   TableView t;
   __host__ __device__ real_t scale() const { return R(1.0); }
   __device__ void begin(size_t) {}
   __device__ void operator()(real_t dx, real_t dy, real_t dz, real_t r2, size_t, real_t& gx, real_t& gy, real_t& gz) const
   {
      real_t e = R(0.0);
      ljTablePair<false>(dx, dy, dz, r2, t, gx, gy, gz, e);
   }
};

// SPLINE: the -P cubic splines in r^2 (drho, dphi are (1/r) d/dr already); else the quadratic tables in r
template <bool SPLINE>
struct VirialEam {
   InterpolationObjectGpu phi, rho;
   InterpolationSplineObjectGpu phiS, rhoS;
   const real_t* __restrict__ dfEmbed;
   real_t dfi;
   __host__ __device__ real_t scale() const { return R(1.0); }
   __device__ void begin(size_t iOff) { dfi = dfEmbed[iOff]; }
   __device__ void operator()(real_t dx, real_t dy, real_t dz, real_t r2, size_t jOff, real_t& gx, real_t& gy, real_t& gz) const
   {
      real_t v, dphi, drho;
      real_t s;
      if (SPLINE) {
         interpolateSpline(phiS, r2, v, dphi);
         interpolateSpline(rhoS, r2, v, drho);
         s = dphi + (dfi + dfEmbed[jOff]) * drho;
      } else {
         const real_t ir = rsqrtR(r2), r = r2 * ir;
         interpolate(makeTable(phi, phi.values), r, v, dphi);
         interpolate(makeTable(rho, rho.values), r, v, drho);
         s = (dphi + (dfi + dfEmbed[jOff]) * drho) * ir;
      }
      gx = -s * dx; gy = -s * dy; gz = -s * dz;
   }
};

template <class PAIR>
__global__ __launch_bounds__(256)
void Virial_thread_atom(VirialArgs v, PAIR pair)
{
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;
   real_t acc[VIRIAL_N];
#pragma unroll
   for (int c = 0; c < VIRIAL_N; ++c) acc[c] = R(0.0);

   forEachChunk(v, lane, wave, [&](int iBox, int first, int, int reps, int, int q, int ia, bool active) {
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
      if (active) {
         const real_t h = R(0.5) * pair.scale();
         acc[0] = fmaR(h, wxx, acc[0]); acc[1] = fmaR(h, wyy, acc[1]); acc[2] = fmaR(h, wzz, acc[2]);
         acc[3] = fmaR(h, wyz, acc[3]); acc[4] = fmaR(h, wxz, acc[4]); acc[5] = fmaR(h, wxy, acc[5]);
      }
      if (active && q == 0) {
         const real_t invMass = R(1.0) / v.speciesMass[v.iSpecies[iOff]];
         const real_t qx = v.px[iOff], qy = v.py[iOff], qz = v.pz[iOff];
         acc[6] = fmaR(qx * qx, invMass, acc[6]); acc[7] = fmaR(qy * qy, invMass, acc[7]); acc[8] = fmaR(qz * qz, invMass, acc[8]);
         acc[9] = fmaR(qy * qz, invMass, acc[9]); acc[10] = fmaR(qx * qz, invMass, acc[10]); acc[11] = fmaR(qx * qy, invMass, acc[11]);
      }
   });
   double sum[VIRIAL_N];
#pragma unroll
   for (int c = 0; c < VIRIAL_N; ++c) sum[c] = (double)acc[c];
   blockSumD(sum, v.partial + (size_t)blockIdx.x * VIRIAL_N);
}

// the rows of partials -> out[VIRIAL_N], in a fixed order
__global__ __launch_bounds__(256)
void Virial_Final(const double* __restrict__ partial, int nPartial, double* __restrict__ out)
{
   double acc[VIRIAL_N];
#pragma unroll
   for (int c = 0; c < VIRIAL_N; ++c) acc[c] = 0.0;
   for (int i = threadIdx.x; i < nPartial; i += blockDim.x)
#pragma unroll
      for (int c = 0; c < VIRIAL_N; ++c) acc[c] += partial[(size_t)i * VIRIAL_N + c];
   blockSumD(acc, out);
}
