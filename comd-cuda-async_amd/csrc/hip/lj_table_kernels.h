// lj_table_kernels.h -- Lennard-Jones by table interpolation (-I) for gfx950.
//
// Same physics as the reference's LJ_Force_thread_atom_interpolation (gpu_lj_thread_atom.h:145-226): the shifted LJ energy
// 4 eps (r6 (r6 - 1) - eShift) tabulated on n = 1000 intervals from sigma/2 to the cutoff (initLJinterpolation, gpu_utility.c:349-372;
// built on the host by comdLjInterpolationTable), read with the quadratic interpolate() of EAM (device_common.h):
//    e_i = sum 1/2 v(r),   f_i = sum -v'(r) / r * d   over 0 < r^2 <= rc^2.
// The table carries the factor 4 eps, so nothing is scaled per atom.
//
// This file holds the pair function and its policy only.  The kernels are the bodies of lj_kernels.h (ljForceThreadAtom) and nl_kernels.h
// (ljForceNlSlabs, ljForceThreadAtomNl) instantiated with LjTablePair: the same walks, lists, replicated tail wave and scalar-load stream as
// the analytic kernels, under kernel names of their own with the TableView as an extra argument.
// The table stays in global memory (an 8 KB array every CU keeps in its L1/L2): each evaluated pair gathers four consecutive samples per lane.
// No LDS copy, so no barrier and nothing in front of the scalar-load stream of the full waves (see the NOTE in ljForceThreadAtom).
#pragma once
#include "device_common.h"
#include "lj_kernels.h"
#include "nl_kernels.h"

// One accepted pair (the reference's per-pair body, gpu_lj_thread_atom.h:197-213): r from r^2 through v_rsq_f64 + Newton, y = 1/r
template <bool ENERGY>
__device__ __forceinline__ void ljTablePair(real_t dx, real_t dy, real_t dz, real_t r2, const TableView& t,
                                            real_t& fx, real_t& fy, real_t& fz, real_t& e)
{
   const real_t y = rsqrtR(r2);
   real_t v, dv;
   interpolate<true>(t, r2 * y, v, dv);
   if (ENERGY) e = fmaR(R(0.5), v, e);
   const real_t fr = -dv * y;
   fx = fmaR(fr, dx, fx); fy = fmaR(fr, dy, fy); fz = fmaR(fr, dz, fz);
}

// the pair policy of -I (see LjAnalyticPair): the table pair, sums stored as they are
struct LjTablePair {
   TableView t;
   template <bool ENERGY>
   __device__ __forceinline__ void pair(const LjArgs&, real_t dx, real_t dy, real_t dz, real_t r2, real_t& fx, real_t& fy, real_t& fz, real_t& e) const
   {
      ljTablePair<ENERGY>(dx, dy, dz, r2, t, fx, fy, fz, e);
   }
   // r^2 in the extra chunks of thread_atom (cells fuller than the grid was sized for, COMD_LJ_WAVES).  Left to -ffp-contract=fast, hipcc rounded it
   // there as fma(dx, dx, dy dy) + dz dz in the float -I kernels when they had a chunk loop of their own, and as fma(dz, dz, dx dx + dy dy) everywhere else,
   // which is also what it chooses for the shared loop.  The float shape is written out so that sharing the loop moved no result; double has one shape.
   __device__ __forceinline__ real_t r2ExtraChunk(real_t dx, real_t dy, real_t dz) const
   {
#ifdef COMD_SINGLE
#pragma clang fp contract(off)
      return fmaR(dx, dx, dy*dy) + dz*dz;
#else
      return dx*dx + dy*dy + dz*dz;
#endif
   }
   template <bool ENERGY>
   __device__ __forceinline__ void store(const LjArgs& a, size_t iOff, real_t fx, real_t fy, real_t fz, real_t e) const
   {
      a.fx[iOff] = fx; a.fy[iOff] = fy; a.fz[iOff] = fz;
      if (ENERGY) a.e[iOff] = e;
   }
};

// thread_atom without the L2 prefetch of the list loop (-I has never had it)
template <bool ENERGY, bool LISTED>
__global__ __launch_bounds__(256)
void LJ_Force_thread_atom_table(LjArgs a, int wavesPerCell, LjWaveLists w, TableView t) { ljForceThreadAtom<LjTablePair, ENERGY, LISTED, false>(LjTablePair{t}, a, wavesPerCell, w); }

template <bool ENERGY>
__global__ __launch_bounds__(512)
void LJ_Force_nl_slabs_table(LjArgs a, NlSlabView nl, int groupAtoms, TableView t) { (void)groupAtoms; ljForceNlSlabs<LjTablePair, ENERGY>(LjTablePair{t}, a, nl); }

template <bool ENERGY>
__global__ __launch_bounds__(256)
void LJ_Force_thread_atom_nl_table(LjArgs a, NlView nl, TableView t) { ljForceThreadAtomNl<LjTablePair, ENERGY>(LjTablePair{t}, a, nl); }
