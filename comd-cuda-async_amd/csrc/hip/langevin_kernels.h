// langevin_kernels.h -- the BAOAB Langevin (NVT) forms of the fused integrator kernels of step_kernels.h.  No counterpart in the reference,
// which integrates NVE only.
//
// Leimkuhler-Matthews BAOAB: B p += (dt/2) f, A r += (dt/2) p/m, O p = c1 p + c2 sqrt(m kB T) xi, A r += (dt/2) p/m, [force], B.
// The two kernels take the places of AdvanceVelocityPosition (first step of a timestep() call: B A O A) and AdvanceVelocityVelocityPosition
// (between steps: B B A O A) with the same cell/lane mapping, the same skin check of the final positions and the same status mirror.
// xi is three standard normals from one Philox4x32-10 call keyed by the seed and counted by (gid, step): Box-Muller in real_t on
// u_i = (x_i + 1/2) 2^-32 (DESIGN.md has the mapping).  Local atoms only; vector loads and stores, no atomics, no LDS, no scratch.
#pragma once
#include "device_common.h"
#include "philox.h"
#include "step_kernels.h"

struct LangevinO { real_t c1, c2, kT; uint32_t key0, key1, step0, step1; };

__device__ __forceinline__ double logR(double x) { return log(x); }
__device__ __forceinline__ float  logR(float x) { return logf(x); }
__device__ __forceinline__ double sqrtR(double x) { return sqrt(x); }
__device__ __forceinline__ float  sqrtR(float x) { return sqrtf(x); }
__device__ __forceinline__ void sincosR(double x, double* s, double* c) { sincos(x, s, c); }
__device__ __forceinline__ void sincosR(float x, float* s, float* c) { sincosf(x, s, c); }
__device__ __forceinline__ double cosR(double x) { return cos(x); }
__device__ __forceinline__ float  cosR(float x) { return cosf(x); }

// three N(0,1) of atom gid at the step of o
__device__ __forceinline__ void langevinNormals(const LangevinO& o, int gid, real_t& xi0, real_t& xi1, real_t& xi2)
{
   const uint32_t ctr[4] = { (uint32_t)gid, o.step0, o.step1, 0u };
   uint32_t x[4];
   comdPhilox4x32_10(ctr, o.key0, o.key1, x);
   const real_t twoPow32 = R(2.3283064365386962890625e-10), twoPi = R(6.283185307179586476925286766559);
   const real_t u0 = ((real_t)x[0] + R(0.5)) * twoPow32, u1 = ((real_t)x[1] + R(0.5)) * twoPow32;
   const real_t u2 = ((real_t)x[2] + R(0.5)) * twoPow32, u3 = ((real_t)x[3] + R(0.5)) * twoPow32;
   const real_t ra = sqrtR(R(-2.0) * logR(u0)), rb = sqrtR(R(-2.0) * logR(u2));
   real_t s, c;
   sincosR(twoPi * u1, &s, &c);
   xi0 = ra * c; xi1 = ra * s; xi2 = rb * cosR(twoPi * u3);
}

// A O A of one atom: r, p in registers after the kicks
// trk (msd_kernels.h): both half drifts count, (dt / 2m) (p before O + p after O), added in real_t and quantised once -- an expression of its own, as in step_kernels.h
__device__ __forceinline__ void langevinAOA(const LangevinO& o, int gid, real_t mass, real_t invMass, real_t dtHalf,
                                            real_t& x, real_t& y, real_t& z, real_t& nx, real_t& ny, real_t& nz, const DispTrack& trk)
{
   real_t ix = R(0.0), iy = R(0.0), iz = R(0.0);
   if (trk.d) { ix = x; iy = y; iz = z; }
   nx += dtHalf * x * invMass; ny += dtHalf * y * invMass; nz += dtHalf * z * invMass;
   real_t xi0, xi1, xi2;
   langevinNormals(o, gid, xi0, xi1, xi2);
   const real_t s = o.c2 * sqrtR(mass * o.kT);
   x = o.c1 * x + s * xi0; y = o.c1 * y + s * xi1; z = o.c1 * z + s * xi2;
   nx += dtHalf * x * invMass; ny += dtHalf * y * invMass; nz += dtHalf * z * invMass;
   if (trk.d) { const real_t w = dtHalf * invMass; dispAdd(trk, gid, w * (ix + x), w * (iy + y), w * (iz + z)); }
}

// B A O A: the first step of a timestep() call
__global__ __launch_bounds__(256)
void AdvanceVelocityPositionLangevin(real_t* __restrict__ rx, real_t* __restrict__ ry, real_t* __restrict__ rz,
                                     real_t* __restrict__ px, real_t* __restrict__ py, real_t* __restrict__ pz,
                                     const real_t* __restrict__ fx, const real_t* __restrict__ fy, const real_t* __restrict__ fz,
                                     const int* __restrict__ iSpecies, const int* __restrict__ gid, const real_t* __restrict__ speciesMass,
                                     const int* __restrict__ nAtoms, int nLocalBoxes, int cap, real_t dtKick, real_t dtHalfDrift, LangevinO o,
                                     SkinCheck sk, DispTrack trk, int laneBits)
{
   skinProgress(sk);
   COMD_CELL_SLOTS(laneBits) {
      const real_t mass = speciesMass[iSpecies[tid]];
      const real_t invMass = R(1.0) / mass;
      real_t x = px[tid] + dtKick * fx[tid], y = py[tid] + dtKick * fy[tid], z = pz[tid] + dtKick * fz[tid];
      real_t nx = rx[tid], ny = ry[tid], nz = rz[tid];
      langevinAOA(o, gid[tid], mass, invMass, dtHalfDrift, x, y, z, nx, ny, nz, trk);
      px[tid] = x; py[tid] = y; pz[tid] = z;
      rx[tid] = nx; ry[tid] = ny; rz[tid] = nz;
      skinCheck(sk, tid, nx, ny, nz);
   }
}

// B B A O A: the closing half kick of one step and the next step up to its force evaluation (the two kicks stay two roundings, as in
// AdvanceVelocityVelocityPosition: a call split in two gives the bits of one call)
__global__ __launch_bounds__(256)
void AdvanceVelocityVelocityPositionLangevin(real_t* __restrict__ rx, real_t* __restrict__ ry, real_t* __restrict__ rz,
                                             real_t* __restrict__ px, real_t* __restrict__ py, real_t* __restrict__ pz,
                                             const real_t* __restrict__ fx, const real_t* __restrict__ fy, const real_t* __restrict__ fz,
                                             const int* __restrict__ iSpecies, const int* __restrict__ gid, const real_t* __restrict__ speciesMass,
                                             const int* __restrict__ nAtoms, int nLocalBoxes, int cap, real_t dtKick1, real_t dtKick2, real_t dtHalfDrift,
                                             LangevinO o, SkinCheck sk, DispTrack trk, int laneBits)
{
   skinProgress(sk);
   COMD_CELL_SLOTS(laneBits) {
      const real_t mass = speciesMass[iSpecies[tid]];
      const real_t invMass = R(1.0) / mass;
      const real_t gx = fx[tid], gy = fy[tid], gz = fz[tid];
      real_t x = px[tid] + dtKick1 * gx, y = py[tid] + dtKick1 * gy, z = pz[tid] + dtKick1 * gz;
      x += dtKick2 * gx; y += dtKick2 * gy; z += dtKick2 * gz;
      real_t nx = rx[tid], ny = ry[tid], nz = rz[tid];
      langevinAOA(o, gid[tid], mass, invMass, dtHalfDrift, x, y, z, nx, ny, nz, trk);
      px[tid] = x; py[tid] = y; pz[tid] = z;
      rx[tid] = nx; ry[tid] = ny; rz[tid] = nz;
      skinCheck(sk, tid, nx, ny, nz);
   }
}
