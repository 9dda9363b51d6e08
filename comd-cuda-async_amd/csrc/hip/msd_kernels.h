// msd_kernels.h -- unwrapped displacements for the mean-squared displacement (comdTrackDisplacementGpu, computeDisplacementSums, comd_hip.h).
// The reference has no counterpart.
//
// State: one 32-byte record per GLOBAL atom id, {dx, dy, dz, spare}, signed 64-bit fixed point in units of 2^-32 Angstroms (resolution
// 2.3e-10 A, range +-2^31 A): the displacement of atom gid since tracking was switched on, as far as THIS rank has drifted it.
// The six drift kernels (step_kernels.h, langevin_kernels.h) add dt p/m -- the motion before any periodic shift -- to the record of the atom
// they move.  An atom is owned by one local slot of one rank at any drift, so one thread owns a gid per drift kernel: plain vector load, add,
// store, no atomics.  The global displacement is the sum of the ranks' records, and a sum of integers does not depend on the order, on the
// number of ranks or on where the atom migrated.  The record is 32 bytes so that an atom's read-modify-write stays inside one sector.
//
// DispTrack is passed by value, as SkinCheck: d == NULL is "not tracking" and dispAdd returns at once.
#pragma once
#include "device_common.h"

struct DispTrack { long long* d; int n; };      // [n][4] records, n = nGlobal

#define COMD_DISP_SCALE 4294967296.0            // 2^32 units per Angstrom

// one drift of atom g by (ix, iy, iz) Angstroms: quantised once, round to nearest.  A gid outside [0, n) (a hole, -1) is not written.
__device__ __forceinline__ void dispAdd(const DispTrack& t, int g, real_t ix, real_t iy, real_t iz)
{
   if ((unsigned)g >= (unsigned)t.n) return;
   long long* __restrict__ r = t.d + 4 * (size_t)g;
   const long long ax = r[0], ay = r[1], az = r[2];
   r[0] = ax + llrint((double)ix * COMD_DISP_SCALE);
   r[1] = ay + llrint((double)iy * COMD_DISP_SCALE);
   r[2] = az + llrint((double)iz * COMD_DISP_SCALE);
}

// ---- sums over the records: stage 1 = per-block partial sums in a fixed order, stage 2 = one block adds the partials (as ReduceEnergy*) --------
// {sum dx, sum dy, sum dz, sum dx^2, sum dy^2, sum dz^2} in Angstroms, in double in both precision builds: int64 -> double is exact below 2^53
// units (2^21 A), then scaled by 2^-32.  No floating-point atomics; the grid is a function of n alone, so the result is reproducible.
#define MSD_BLOCKS 1024
#define MSD_N 6

__global__ __launch_bounds__(256)
void ReduceDisplacementPartial(const long long* __restrict__ d, int n, double* __restrict__ partial)
{
   double acc[MSD_N];
#pragma unroll
   for (int c = 0; c < MSD_N; ++c) acc[c] = 0.0;
   const double unit = 1.0 / COMD_DISP_SCALE;
   for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long)gridDim.x * blockDim.x) {
      const long long* __restrict__ r = d + 4 * (size_t)g;
      const double x = (double)r[0] * unit, y = (double)r[1] * unit, z = (double)r[2] * unit;
      acc[0] += x; acc[1] += y; acc[2] += z;
      acc[3] += x * x; acc[4] += y * y; acc[5] += z * z;
   }
   blockSumD(acc, partial + (size_t)MSD_N * blockIdx.x);
}

__global__ __launch_bounds__(256)
void ReduceDisplacementFinal(const double* __restrict__ partial, int nPartial, double* __restrict__ out)
{
   double acc[MSD_N];
#pragma unroll
   for (int c = 0; c < MSD_N; ++c) acc[c] = 0.0;
   for (int i = threadIdx.x; i < nPartial; i += blockDim.x)
#pragma unroll
      for (int c = 0; c < MSD_N; ++c) acc[c] += partial[(size_t)MSD_N * i + c];
   blockSumD(acc, out);
}
