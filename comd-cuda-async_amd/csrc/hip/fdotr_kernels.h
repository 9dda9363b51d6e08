// fdotr_kernels.h -- the pair virial from the forces the step has already left on the device (computeVirialFdotr, comd_hip.h): what a barostat can afford
// inside the step loop.  The reference has no counterpart.
//
// With f_ij = -f_ji the force on i due to j, F_i = sum_j f_ij the total force of a local atom (j over local atoms and halo images) and the stored position of a
// halo image r_j + s_ij (s_ij the periodic shift of its halo cell), the virial of virial_kernels.h is, exactly,
//   W_ab = 1/2 sum_i sum_j (r_i - r_j - s_ij)_a f_ij,b = sum_i r_i,a F_i,b  -  1/2 sum_(i local, j an image across a PERIODIC face) s_ij,a f_ij,b
// (sum_i sum_j r_j f_ij = -sum_j r_j F_j: every pair is seen from both sides, on two ranks when it straddles a rank boundary).  A halo cell that is no periodic
// wrap has s = 0 and contributes nothing.  The identity needs "halo position = home position + shift of that halo cell" only, so it holds for the cells of the
// *_nl methods, which are not re-binned between list builds.  Off-diagonals are symmetrised, 1/2 (a_y b_z + a_z b_y): the exact tensor is symmetric.
//
//   Fdotr_atoms  one pass over the occupied slots of the local cells in the launch shape of the integrator kernels (2^laneBits lanes per cell): r (x) F with r taken
//                about the centre of the global box -- sum_i F_i is zero to rounding only, and the centre halves what that residue is multiplied by -- and
//                K_ab = p_a p_b / m with the expressions of Virial_thread_atom.  One row of 12 partials per workgroup.
//   Fdotr_face   over a work list of rows (local cell, periodic halo cell, sign_x, sign_y, sign_z), s_a = sign_a L_a, built once on the host from the static
//                neighbour table (comdPeriodicFacePairs).  A wave takes a row: the atoms of the local cell, replicated as the chunks of stencil_walk.h are
//                (copy q takes the atoms q, q + reps, ... of the halo cell), against the atoms of that one halo cell, with the acceptance test and the pair
//                functors of Virial_thread_atom (EAM reads F'_j from dfEmbed's halo slots).  A lane sums f_ij over the halo cell and adds -1/2 s_a f_b.
//                L is an argument of every launch: the box changes.  One row of 12 partials (the kinetic half 0) per workgroup.
//   Virial_Final adds all rows in a fixed order.
// Lanes accumulate in real_t, workgroups sum in double in a fixed order (blockSumD); no atomics, fixed grids: bit-reproducible.  The kernels read r, f, p, dfEmbed
// and the cell tables and write nothing but their own partial rows.
#pragma once
#include "virial_kernels.h"

#define FDOTR_FACE_BLOCKS 2048         // rows of partials of the face kernel: fixed, so the order of the sums does not depend on the system

struct FdotrAtomsArgs {
   const real_t* __restrict__ rx; const real_t* __restrict__ ry; const real_t* __restrict__ rz;
   const real_t* __restrict__ fx; const real_t* __restrict__ fy; const real_t* __restrict__ fz;
   const real_t* __restrict__ px; const real_t* __restrict__ py; const real_t* __restrict__ pz;
   const int* __restrict__ iSpecies; const real_t* __restrict__ speciesMass;
   const int* __restrict__ nAtoms;
   int nLocalBoxes, cap, laneBits;
   real_t cx, cy, cz;                  // centre of the global box
   double* __restrict__ partial;       // [gridDim.x][VIRIAL_N]
};

__global__ __launch_bounds__(256)
void Fdotr_atoms(FdotrAtomsArgs v)
{
   real_t acc[VIRIAL_N];
#pragma unroll
   for (int c = 0; c < VIRIAL_N; ++c) acc[c] = R(0.0);
   const int cell = (int)blockIdx.x * (256 >> v.laneBits) + ((int)threadIdx.x >> v.laneBits);
   if (cell < v.nLocalBoxes) {
      const real_t h = R(0.5);
      for (long tid = (long)cell * v.cap + ((int)threadIdx.x & ((1 << v.laneBits) - 1)), tidEnd = (long)cell * v.cap + v.nAtoms[cell]; tid < tidEnd; tid += (1 << v.laneBits)) {
         const real_t x = v.rx[tid] - v.cx, y = v.ry[tid] - v.cy, z = v.rz[tid] - v.cz;
         const real_t gx = v.fx[tid], gy = v.fy[tid], gz = v.fz[tid];
         acc[0] = fmaR(x, gx, acc[0]); acc[1] = fmaR(y, gy, acc[1]); acc[2] = fmaR(z, gz, acc[2]);
         acc[3] = fmaR(h, fmaR(y, gz, z * gy), acc[3]); acc[4] = fmaR(h, fmaR(x, gz, z * gx), acc[4]); acc[5] = fmaR(h, fmaR(x, gy, y * gx), acc[5]);
         const real_t invMass = R(1.0) / v.speciesMass[v.iSpecies[tid]];
         const real_t qx = v.px[tid], qy = v.py[tid], qz = v.pz[tid];
         acc[6] = fmaR(qx * qx, invMass, acc[6]); acc[7] = fmaR(qy * qy, invMass, acc[7]); acc[8] = fmaR(qz * qz, invMass, acc[8]);
         acc[9] = fmaR(qy * qz, invMass, acc[9]); acc[10] = fmaR(qx * qz, invMass, acc[10]); acc[11] = fmaR(qx * qy, invMass, acc[11]);
      }
   }
   double sum[VIRIAL_N];
#pragma unroll
   for (int c = 0; c < VIRIAL_N; ++c) sum[c] = (double)acc[c];
   blockSumD(sum, v.partial + (size_t)blockIdx.x * VIRIAL_N);
}

struct FdotrFaceArgs {
   const real_t* __restrict__ rx; const real_t* __restrict__ ry; const real_t* __restrict__ rz;
   const int* __restrict__ nAtoms;
   const int* __restrict__ rows;       // [nRows][5]: local cell, periodic halo cell, sign x y z
   int nRows, cap;
   real_t rc2;
   real_t lx, ly, lz;                  // the global extents of this launch
   double* __restrict__ partial;       // [gridDim.x][VIRIAL_N]
};

template <class PAIR>
__global__ __launch_bounds__(256)
void Fdotr_face(FdotrFaceArgs v, PAIR pair)
{
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;
   real_t wxx = R(0.0), wyy = R(0.0), wzz = R(0.0), wyz = R(0.0), wxz = R(0.0), wxy = R(0.0);
   const long per = ((long)v.nRows + gridDim.x - 1) / gridDim.x;
   const long w0 = (long)xcdRemap(blockIdx.x, gridDim.x) * per;
   const long w1 = w0 + per < v.nRows ? w0 + per : v.nRows;
   for (long w = w0 + wave; w < w1; w += 4) {
      const int* __restrict__ row = v.rows + 5 * w;
      const int iBox = uniform(row[0]), jBox = uniform(row[1]);
      const int ni = uniform(v.nAtoms[iBox]), nj = uniform(v.nAtoms[jBox]);
      if (ni == 0 || nj == 0) continue;
      // -1/2 s_a, s_a = sign_a L_a
      const real_t ax = R(-0.5) * (real_t)uniform(row[2]) * v.lx, ay = R(-0.5) * (real_t)uniform(row[3]) * v.ly, az = R(-0.5) * (real_t)uniform(row[4]) * v.lz;
      const size_t jBase = (size_t)jBox * v.cap;
      for (int first = 0; first < ni; first += WAVE) {
         const int m = ni - first < WAVE ? ni - first : WAVE;
         int reps = 1;
         while (2 * reps * m <= WAVE) reps *= 2;
         const int span = WAVE / reps, q = lane / span;
         const int ia = first + (lane & (span - 1));
         const bool active = ia < first + m;
         const size_t iOff = (size_t)iBox * v.cap + (active ? ia : first);
         const real_t xi = v.rx[iOff], yi = v.ry[iOff], zi = v.rz[iOff];
         pair.begin(iOff);
         real_t sx = R(0.0), sy = R(0.0), sz = R(0.0);
         for (int j = q; j < nj; j += reps) {
            const size_t jOff = jBase + j;
            const real_t dx = xi - v.rx[jOff], dy = yi - v.ry[jOff], dz = zi - v.rz[jOff];
            const real_t r2 = dx*dx + dy*dy + dz*dz;
            if (active && r2 <= v.rc2 && r2 > R(0.0)) {
               real_t gx = R(0.0), gy = R(0.0), gz = R(0.0);
               pair(dx, dy, dz, r2, jOff, gx, gy, gz);
               sx += gx; sy += gy; sz += gz;
            }
         }
         if (active) {
            const real_t s = pair.scale(), h = R(0.5);
            sx *= s; sy *= s; sz *= s;
            wxx = fmaR(ax, sx, wxx); wyy = fmaR(ay, sy, wyy); wzz = fmaR(az, sz, wzz);
            wyz = fmaR(h, fmaR(ay, sz, az * sy), wyz); wxz = fmaR(h, fmaR(ax, sz, az * sx), wxz); wxy = fmaR(h, fmaR(ax, sy, ay * sx), wxy);
         }
      }
   }
   double sum[VIRIAL_N];
   sum[0] = (double)wxx; sum[1] = (double)wyy; sum[2] = (double)wzz; sum[3] = (double)wyz; sum[4] = (double)wxz; sum[5] = (double)wxy;
#pragma unroll
   for (int c = 6; c < VIRIAL_N; ++c) sum[c] = 0.0;
   blockSumD(sum, v.partial + (size_t)blockIdx.x * VIRIAL_N);
}
