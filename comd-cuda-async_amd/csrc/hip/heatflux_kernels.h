// heatflux_kernels.h -- the per-atom heat flux for gfx950 (computeHeatFlux, comd_hip.h).  The reference has no counterpart.
//
// For every local atom i, with v_i = p_i / m_i, nine components in the order jk x y z, jp x y z, jv x y z, in eV A/fs (flux density x volume):
//   jk_i = (|p_i|^2 / 2 m_i) v_i                    kinetic convective part
//   jp_i = e_i v_i                                  potential convective part, e_i the per-atom energy the force kernels have left in e[]
//   jv_i = 1/2 sum_j r_ij (f_ij . v_i)              virial part: -s_i v_i with s_i the pair part of stress_kernels.h
// j over the neighbours (local or halo image) with 0 < |r_ij|^2 <= rc^2, r_ij = r_i - r_j, f_ij the force on i due to j: the pair convention of
// virial_kernels.h -- its acceptance test, its functors (EAM reads F'_j from dfEmbed, halo slots included), each pair weighing 1/2 on either side.
// The virial part is one-sided: summed over i it is 1/2 sum_{i<j} r_ij f_ij . (v_i + v_j), but an atom needs its OWN velocity only, so no lane reads
// the momentum of a halo slot, which the halo exchange does not keep current between redistributions.
//
// Mapping: the chunk walk of stencil_walk.h, lane = atom i; v_i is formed once per atom, and per accepted pair the lane forms c = (f_ij / scale) . v_i
// and adds d c to three sums in real_t: one dot product and three accumulators where the tensor of stress_kernels.h takes six.  The copies of a
// replicated chunk are added by sumOverCopies; copy 0 forms the nine components.
//   STORE = true   nine SoA planes [9][nLocalBoxes*cap] of real_t: consecutive lanes store consecutive slots of a plane; no rows are written.
//   STORE = false  the sampled path: every lane adds the components of its atoms in real_t, the workgroup sums them in double in a fixed order
//                  (blockSumD) into one row of 9; HeatFlux_Final adds the rows in a fixed order.  Nothing per atom is written.
// No atomics, no LDS beyond blockSumD, no scratch; bit-reproducible.  The kernel reads r, p, e, dfEmbed, species and the cell tables and writes
// nothing but its planes or its rows.
#pragma once
#include "virial_kernels.h"

#define HEATFLUX_N 9                   // jk, jp, jv: three components each
#define HEATFLUX_BLOCKS 2048           // the grid of the walk and the rows of partials, as VIRIAL_BLOCKS: fixed, so the order of the sums does not depend on the system

struct HeatFluxArgs : StencilArgs {
   const real_t* __restrict__ px; const real_t* __restrict__ py; const real_t* __restrict__ pz;
   const real_t* __restrict__ e;
   const int* __restrict__ iSpecies; const real_t* __restrict__ speciesMass;
   real_t rc2;
   size_t plane;                       // nLocalBoxes * cap: the slots of one plane of the output
};

// out: [9][plane] (STORE) or unused; partial: [gridDim.x][HEATFLUX_N] (!STORE) or unused.  Both are kernel parameters of their own, __restrict__: the planes are
// stored inside the loop over the chunks, and only the noalias of a parameter keeps the scalar-load stream of the full chunks (stress_kernels.h).
template <class PAIR, bool STORE>
__global__ __launch_bounds__(256)
void HeatFlux_thread_atom(HeatFluxArgs v, PAIR pair, real_t* __restrict__ out, double* __restrict__ partial)
{
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;
   real_t acc[HEATFLUX_N];
#pragma unroll
   for (int c = 0; c < HEATFLUX_N; ++c) acc[c] = R(0.0);

   forEachChunk(v, lane, wave, [&](int iBox, int first, int, int reps, int span, int q, int ia, bool active) {
      const size_t iOff = (size_t)iBox * v.cap + (active ? ia : first);
      const real_t xi = v.rx[iOff], yi = v.ry[iOff], zi = v.rz[iOff];
      const real_t mass = v.speciesMass[v.iSpecies[iOff]];
      const real_t qx = v.px[iOff], qy = v.py[iOff], qz = v.pz[iOff];
      const real_t vx = qx / mass, vy = qy / mass, vz = qz / mass;
      pair.begin(iOff);
      real_t sx = R(0.0), sy = R(0.0), sz = R(0.0);
      auto test = [&](real_t xj, real_t yj, real_t zj, size_t jOff) {
         const real_t dx = xi - xj, dy = yi - yj, dz = zi - zj;
         const real_t r2 = dx*dx + dy*dy + dz*dz;
         if (active && r2 <= v.rc2 && r2 > R(0.0)) {
            real_t gx = R(0.0), gy = R(0.0), gz = R(0.0);
            pair(dx, dy, dz, r2, jOff, gx, gy, gz);
            const real_t c = fmaR(gz, vz, fmaR(gy, vy, gx * vx));
            sx = fmaR(dx, c, sx); sy = fmaR(dy, c, sy); sz = fmaR(dz, c, sz);
         }
      };
      stencilWalk<size_t>(v, iBox, reps, q, test);
      if (reps > 1) sumOverCopies(lane, span, sx, sy, sz);
      if (active && q == 0) {
         // every product is rounded on its own in both instances, so the sampled path adds the very values the planes hold
#pragma clang fp contract(off)
         const real_t h = R(0.5) * pair.scale();
         const real_t ke = R(0.5) * fmaR(qz, vz, fmaR(qy, vy, qx * vx));
         const real_t ei = v.e[iOff];
         const real_t j[HEATFLUX_N] = { ke * vx, ke * vy, ke * vz, ei * vx, ei * vy, ei * vz, h * sx, h * sy, h * sz };
         if (STORE) {
            real_t* __restrict__ o = out + iOff;
#pragma unroll
            for (int c = 0; c < HEATFLUX_N; ++c) o[c * v.plane] = j[c];
         } else {
#pragma unroll
            for (int c = 0; c < HEATFLUX_N; ++c) acc[c] += j[c];
         }
      }
   });
   if (!STORE) {
      double sum[HEATFLUX_N];
#pragma unroll
      for (int c = 0; c < HEATFLUX_N; ++c) sum[c] = (double)acc[c];
      blockSumD(sum, partial + (size_t)blockIdx.x * HEATFLUX_N);
   }
}

// the rows of partials -> out[HEATFLUX_N], in a fixed order
__global__ __launch_bounds__(256)
void HeatFlux_Final(const double* __restrict__ partial, int nPartial, double* __restrict__ out)
{
   double acc[HEATFLUX_N];
#pragma unroll
   for (int c = 0; c < HEATFLUX_N; ++c) acc[c] = 0.0;
   for (int i = threadIdx.x; i < nPartial; i += blockDim.x)
#pragma unroll
      for (int c = 0; c < HEATFLUX_N; ++c) acc[c] += partial[(size_t)i * HEATFLUX_N + c];
   blockSumD(acc, out);
}
