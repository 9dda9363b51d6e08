// deform_kernels.h -- box deformation (not in the reference, whose box is fixed at nx lat for the whole run): the affine remap of the positions to a new box,
// what LAMMPS calls `fix deform ... remap x`.
//
// r_a <- r_a * scale_a about the global origin (globalMin is 0 on every axis) for the atoms in the occupied slots of the LOCAL cells; momenta are not touched
// (remap x, not remap v), halo cells are not touched (the redistribution that always follows refills them) and neither are the displacement records of
// msd_kernels.h: the MSD stays the non-affine displacement.  With Verlet lists the same pass scales the build-time snapshot lastR by the same factors, so that the
// skin test of the drift kernels (step_kernels.h SkinCheck) keeps measuring the non-affine motion since the build only.
// One read-modify-write of r (and of lastR): memory-bound, no atomics, no LDS, the launch shape of the slot-wise integrator kernels.
#pragma once
#include "device_common.h"
#include "step_kernels.h"

struct RemapSnapshot { real_t* x; real_t* y; real_t* z; };      // lastR of the Verlet lists, x == NULL: none

__global__ __launch_bounds__(256)
void RemapBox(real_t* __restrict__ rx, real_t* __restrict__ ry, real_t* __restrict__ rz, RemapSnapshot last,
              const int* __restrict__ nAtoms, int nLocalBoxes, int cap, real_t sx, real_t sy, real_t sz, int laneBits)
{
   COMD_CELL_SLOTS(laneBits) {
      rx[tid] *= sx; ry[tid] *= sy; rz[tid] *= sz;
      if (last.x) { last.x[tid] *= sx; last.y[tid] *= sy; last.z[tid] *= sz; }
   }
}
