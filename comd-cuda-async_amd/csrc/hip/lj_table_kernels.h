// lj_table_kernels.h -- Lennard-Jones by table interpolation (-I) for gfx950.
//
// Same physics as the reference's LJ_Force_thread_atom_interpolation (gpu_lj_thread_atom.h:145-226): the shifted LJ energy
// 4 eps (r6 (r6 - 1) - eShift) tabulated on n = 1000 intervals from sigma/2 to the cutoff (initLJinterpolation, gpu_utility.c:349-372;
// built on the host by comdLjInterpolationTable), read with the quadratic interpolate() of EAM (device_common.h):
//    e_i = sum 1/2 v(r),   f_i = sum -v'(r) / r * d   over 0 < r^2 <= rc^2.
// The table carries the factor 4 eps, so nothing is scaled per atom.
//
// The machine mappings are those of the analytic kernels, restated with the table pair in place of ljPair (lj_kernels.h and
// nl_kernels.h stay as they are; everything in them that does not depend on the pair function is used from there):
//   LJ_Force_thread_atom_table  : LJ_Force_thread_atom -- a wave per 64-slot chunk of a cell, j wave-uniform through the scalar unit,
//                                 the wave candidate lists of LJ_WaveCandidates with the stencil walk as fallback, the replicated tail wave.
//   LJ_Force_nl_slabs_table     : LJ_Force_nl_slabs -- workgroup per cell, 16-bit rows into the LDS staging of a group of 9 stencil cells.
//   LJ_Force_thread_atom_nl_table : LJ_Force_thread_atom_nl -- thread per slot over the global-slot lists (the other list format).
// The table stays in global memory (an 8 KB array every CU keeps in its L1/L2): each evaluated pair gathers four consecutive samples per lane.
// No LDS copy, so no barrier and nothing in front of the scalar-load stream of the full waves (see the NOTE in LJ_Force_thread_atom).
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

// ljCellLoop with the table pair: one neighbour cell against the wave's 64 i atoms, 8 wave-uniform neighbours per scalar-load batch
template <bool SELF, bool ENERGY>
__device__ __forceinline__ void ljTableCellLoop(const LjArgs& a, const TableView& t, int jBox, real_t xi, real_t yi, real_t zi,
                                                real_t& fx, real_t& fy, real_t& fz, real_t& e)
{
   const int nj = uniform(a.nAtoms[jBox]);
   const real_t* __restrict__ px = a.rx + (size_t)jBox * a.cap;
   const real_t* __restrict__ py = a.ry + (size_t)jBox * a.cap;
   const real_t* __restrict__ pz = a.rz + (size_t)jBox * a.cap;
   int j = 0;
   for (; j + 8 <= nj; j += 8) {
      real_t xs[8], ys[8], zs[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { xs[u] = px[j + u]; ys[u] = py[j + u]; zs[u] = pz[j + u]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
         real_t dx = xi - xs[u], dy = yi - ys[u], dz = zi - zs[u];
         real_t r2 = dx*dx + dy*dy + dz*dz;
         bool hit = SELF ? (r2 <= a.rc2 && r2 > R(0.0)) : (r2 <= a.rc2);
         if (hit) ljTablePair<ENERGY>(dx, dy, dz, r2, t, fx, fy, fz, e);
      }
   }
   for (; j < nj; ++j) {
      real_t dx = xi - px[j], dy = yi - py[j], dz = zi - pz[j];
      real_t r2 = dx*dx + dy*dy + dz*dz;
      bool hit = SELF ? (r2 <= a.rc2 && r2 > R(0.0)) : (r2 <= a.rc2);
      if (hit) ljTablePair<ENERGY>(dx, dy, dz, r2, t, fx, fy, fz, e);
   }
}

// ljListLoop with the table pair: eight list offsets per s_load_dwordx8, one s_load_dwordx8 per candidate record, the offsets of the next
// batch fetched with the records of this one
template <bool SELF, bool ENERGY>
__device__ __forceinline__ void ljTableListLoop(const TableView& t, const LjPos4* __restrict__ pos, const unsigned* __restrict__ L, int p, int pEnd,
                                                real_t xi, real_t yi, real_t zi, real_t& fx, real_t& fy, real_t& fz, real_t& e)
{
   auto test = [&](const LjPos4& q) {
      real_t dx = xi - q.x, dy = yi - q.y, dz = zi - q.z;
      real_t r2 = dx*dx + dy*dy + dz*dz;
      bool hit = SELF ? (r2 <= q.rc2 && r2 > R(0.0)) : (r2 <= q.rc2);        // (the record's own copy of rc^2: see LjPos4)
      if (hit) ljTablePair<ENERGY>(dx, dy, dz, r2, t, fx, fy, fz, e);
   };
   const int n8 = (pEnd - p) >> 3;
   if (n8 > 0) {
      const int last = p + 8 * (n8 - 1);
      unsigned id[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) id[u] = L[p + u];
      for (int b = 0; b < n8; ++b, p += 8) {
         LjPos4 q[8];
         unsigned idn[8];
         const int pn = p + 8 < last ? p + 8 : last;
#pragma unroll
         for (int u = 0; u < 8; ++u) q[u] = atByte(pos, id[u]);
#pragma unroll
         for (int u = 0; u < 8; ++u) idn[u] = L[pn + u];
#pragma unroll
         for (int u = 0; u < 8; ++u) test(q[u]);
#pragma unroll
         for (int u = 0; u < 8; ++u) id[u] = idn[u];
      }
   }
   for (; p < pEnd; ++p) test(atByte(pos, L[p]));
}

// the replicas of an under-filled wave meet through ds_bpermute; lanes < m store their atom (no constant factors: the table has them)
template <bool ENERGY>
__device__ __forceinline__ void ljTableChunkStore(const LjArgs& a, size_t iOff, int m, int G, int ai, int lane, real_t fx, real_t fy, real_t fz, real_t e)
{
   real_t tx = fx, ty = fy, tz = fz, te = e;
   for (int r = 1; r < G; ++r) {                       // all lanes take part; only lanes < m keep the result
      const int src = (ai + r * m) & 63;
      tx += bpermuteR(fx, src); ty += bpermuteR(fy, src); tz += bpermuteR(fz, src);
      if (ENERGY) te += bpermuteR(e, src);
   }
   if (lane < m) {
      a.fx[iOff] = tx; a.fy[iOff] = ty; a.fz[iOff] = tz;
      if (ENERGY) a.e[iOff] = te;
   }
}

// ljChunkGeneric with the table pair: m <= 64 atoms replicated G = 64/m (<= 4) times, replica g takes the stencil cells g, g+G, ...
template <bool ENERGY>
__device__ __forceinline__ void ljTableChunkGeneric(const LjArgs& a, const TableView& t, int iBox, int ni, int chunk, int lane)
{
   const int* __restrict__ nb = a.nbr + (size_t)iBox * 27;
   const int m = ni - chunk * 64 < 64 ? ni - chunk * 64 : 64;
   const int G = 64 / m < 4 ? 64 / m : 4;
   const int g = lane / m, ai = lane - g * m;
   const bool valid = g < G;
   const size_t iOff = (size_t)iBox * a.cap + chunk * 64 + (valid ? ai : 0);
   const real_t xi = a.rx[iOff], yi = a.ry[iOff], zi = a.rz[iOff];
   real_t fx = R(0.0), fy = R(0.0), fz = R(0.0), e = R(0.0);
   for (int tr = 0; tr * G < 27; ++tr) {
      const int k = tr * G + g;
      const bool okk = valid && k < 27;
      const int jBox = okk ? nb[k] : iBox;
      const int nj = okk ? a.nAtoms[jBox] : 0;
      const size_t base = (size_t)jBox * a.cap;
      for (int j = 0; __any(j < nj); ++j) {
         if (j < nj) {
            const real_t dx = xi - a.rx[base + j], dy = yi - a.ry[base + j], dz = zi - a.rz[base + j];
            const real_t r2 = dx*dx + dy*dy + dz*dz;
            if (r2 <= a.rc2 && r2 > R(0.0)) ljTablePair<ENERGY>(dx, dy, dz, r2, t, fx, fy, fz, e);
         }
      }
   }
   ljTableChunkStore<ENERGY>(a, iOff, m, G, ai, lane, fx, fy, fz, e);
}

// ljChunkListed with the table pair: replica g takes the g-th part of the wave's candidate list (parts of a multiple of four entries)
template <bool ENERGY>
__device__ __forceinline__ void ljTableChunkListed(const LjArgs& a, const TableView& t, const LjPos4* __restrict__ pos, const unsigned* __restrict__ L,
                                                   int nAll, int iBox, int ni, int chunk, int lane)
{
   const int m = ni - chunk * 64 < 64 ? ni - chunk * 64 : 64;
   const int G = 64 / m < 4 ? 64 / m : 4;
   const int g = lane / m, ai = lane - g * m;
   const bool valid = g < G;
   const size_t iOff = (size_t)iBox * a.cap + chunk * 64 + (valid ? ai : 0);
   const real_t xi = a.rx[iOff], yi = a.ry[iOff], zi = a.rz[iOff];
   real_t fx = R(0.0), fy = R(0.0), fz = R(0.0), e = R(0.0);
   const int len = (((nAll + G - 1) / G) + 3) & ~3;          // entries per replica
   const int first = valid ? g * len : nAll;
   const int mine = nAll - first < len ? nAll - first : len;  // may be <= 0
   const uint4* __restrict__ L4 = reinterpret_cast<const uint4*>(L + (valid ? first : 0));
   for (int it = 0; it < len; it += 4) {
      const bool on = it < mine;
      const uint4 id = on ? L4[it >> 2] : make_uint4(0u, 0u, 0u, 0u);
      const unsigned ids[4] = { id.x, id.y, id.z, id.w };
      LjPos4 q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = atByte(pos, it + u < mine ? ids[u] : 0u);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
         const real_t dx = xi - q[u].x, dy = yi - q[u].y, dz = zi - q[u].z;
         const real_t r2 = dx*dx + dy*dy + dz*dz;
         if (it + u < mine && r2 <= a.rc2 && r2 > R(0.0)) ljTablePair<ENERGY>(dx, dy, dz, r2, t, fx, fy, fz, e);
      }
   }
   ljTableChunkStore<ENERGY>(a, iOff, m, G, ai, lane, fx, fy, fz, e);
}

// ---------------------------------------------------------------------------------------------------
// LJ_Force_thread_atom with the table pair.  Same grid (one workgroup of wavesPerCell waves per cell, or 4-wave workgroups laid flat over
// (cell, chunk)), same lists, same fallbacks; the table is an extra argument, LjArgs is the analytic kernel's.
template <bool ENERGY, bool LISTED>
__global__ __launch_bounds__(256)
void LJ_Force_thread_atom_table(LjArgs a, int wavesPerCell, LjWaveLists w, TableView t)
{
   const int lane = threadIdx.x & 63;
   const int gw = uniform(xcdRemap(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + (threadIdx.x >> 6));
   const int ci = gw / wavesPerCell;
   const int chunk = gw - ci * wavesPerCell;
   if (ci >= a.nCells) return;
   const int iBox = uniform(a.cells ? a.cells[ci] : ci);
   const int ni = uniform(a.nAtoms[iBox]);
   if (chunk * 64 >= ni) return;
   const int m = uniform(ni - chunk * 64 < 64 ? ni - chunk * 64 : 64);     // atoms this wave owns

   int nSelf = 0, nAll = -1;                                                // this wave's candidate list, if it has one
   if (LISTED && chunk < w.wavesMax) {
      const int2 c = w.count[iBox * w.wavesMax + chunk];
      nSelf = uniform(c.x); nAll = uniform(c.y);
   }
   const unsigned* __restrict__ L = LISTED ? w.cand + (size_t)(iBox * w.wavesMax + chunk) * w.candCap : nullptr;
   if (m <= 32) {
      if (LISTED && nAll >= 0) ljTableChunkListed<ENERGY>(a, t, w.pos, L, nAll, iBox, ni, chunk, lane);
      else                     ljTableChunkGeneric<ENERGY>(a, t, iBox, ni, chunk, lane);
   } else {
      // full wave: neighbour j is wave-uniform -> positions arrive through the scalar unit
      const int* __restrict__ nb = a.nbr + (size_t)iBox * 27;
      const int iSlot = chunk * 64 + lane;
      const bool active = iSlot < ni;
      const size_t iOff = (size_t)iBox * a.cap + (active ? iSlot : ni - 1);   // idle lanes shadow the last atom
      const real_t xi = a.rx[iOff], yi = a.ry[iOff], zi = a.rz[iOff];
      real_t fx = R(0.0), fy = R(0.0), fz = R(0.0), e = R(0.0);
      if (LISTED && nAll >= 0) {
         ljTableListLoop<true, ENERGY>(t, w.pos, L, 0, nSelf, xi, yi, zi, fx, fy, fz, e);
         ljTableListLoop<false, ENERGY>(t, w.pos, L, nSelf, nAll, xi, yi, zi, fx, fy, fz, e);
      } else {
         ljTableCellLoop<true, ENERGY>(a, t, iBox, xi, yi, zi, fx, fy, fz, e);
         for (int k = 1; k < 27; ++k) ljTableCellLoop<false, ENERGY>(a, t, uniform(nb[k]), xi, yi, zi, fx, fy, fz, e);
      }
      if (active) {
         a.fx[iOff] = fx; a.fy[iOff] = fy; a.fz[iOff] = fz;
         if (ENERGY) a.e[iOff] = e;
      }
   }
   // (as in LJ_Force_thread_atom: no store ahead of the scalar-path loads above; the extra chunks run after the first one is stored)
   for (int c = chunk + wavesPerCell; c * 64 < ni; c += wavesPerCell) ljTableChunkGeneric<ENERGY>(a, t, iBox, ni, c, lane);
}

// ---------------------------------------------------------------------------------------------------
// LJ_Force_nl_slabs with the table pair: workgroup per cell, thread per atom (replicated tail wave), one group of 9 stencil cells staged in
// the LDS at a time, the 16-bit rows of the slab-format Verlet lists read NL_BATCH at a time.  The lists hold no self entry: no r2 > 0 guard.
template <bool ENERGY>
__global__ __launch_bounds__(512)
void LJ_Force_nl_slabs_table(LjArgs a, NlSlabView nl, int groupAtoms, TableView t)
{
   extern __shared__ __attribute__((aligned(16))) real_t ldsPos[];      // {x, y, z} records
   real_t* __restrict__ sp = ldsPos;
   (void)groupAtoms;
   const int iBox = a.cells ? a.cells[blockIdx.x] : blockIdx.x;
   const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
   const int ni = uniform(a.nAtoms[iBox]);
   const int m = ni - 64 * wave < 64 ? (ni - 64 * wave > 0 ? ni - 64 * wave : 0) : 64;
   const int G = (m > 0 && m <= 32) ? (64 / m < 4 ? 64 / m : 4) : 1;
   const int g = G > 1 ? lane / m : 0, ai = G > 1 ? lane - g * m : lane;
   const int i = 64 * wave + ai;                              // the atom of this lane
   const bool active = ai < m && g < G;
   const size_t iSlot = (size_t)iBox * a.cap + (active ? i : 0);
   const real_t xi = a.rx[iSlot], yi = a.ry[iSlot], zi = a.rz[iSlot];
   real_t fx = R(0.0), fy = R(0.0), fz = R(0.0), e = R(0.0);
   for (int grp = 0; grp < NL_GROUPS; ++grp) {
      if (grp) __syncthreads();                       // everyone is done reading the previous group
      {
         real_t vx[NL_GROUP_CELLS], vy[NL_GROUP_CELLS], vz[NL_GROUP_CELLS];
         int dst[NL_GROUP_CELLS];
         int off = 0;
#pragma unroll
         for (int kk = 0; kk < NL_GROUP_CELLS; ++kk) {
            const int jBox = a.nbr[(size_t)iBox * 27 + groupCell(grp, kk)];
            const int nj = a.nAtoms[jBox];
            const size_t js = (size_t)jBox * a.cap + (tid < nj ? tid : 0);
            vx[kk] = a.rx[js]; vy[kk] = a.ry[js]; vz[kk] = a.rz[js];
            dst[kk] = tid < nj ? off + tid : -1;
            off += nj;
         }
#pragma unroll
         for (int kk = 0; kk < NL_GROUP_CELLS; ++kk)
            if (dst[kk] >= 0) { sp[3 * dst[kk]] = vx[kk]; sp[3 * dst[kk] + 1] = vy[kk]; sp[3 * dst[kk] + 2] = vz[kk]; }
      }
      __syncthreads();
      if (active) {
         const int nAll = nl.count[(size_t)(iBox * NL_GROUPS + grp) * a.cap + i];
         const int n = nAll > g ? (nAll - g + G - 1) / G : 0;               // rows of this replica: g, g + G, ...
         const unsigned short* __restrict__ row = nl.list + ((size_t)(iBox * NL_GROUPS + grp) * nl.rows + g) * a.cap + i;
         const size_t step = (size_t)G * a.cap;
         int k = 0;
         int jn[NL_BATCH];
         if (n >= NL_BATCH) {
#pragma unroll
            for (int u = 0; u < NL_BATCH; ++u) jn[u] = row[(size_t)u * step];
         }
         for (; k + NL_BATCH <= n; k += NL_BATCH) {
            int j[NL_BATCH];
#pragma unroll
            for (int u = 0; u < NL_BATCH; ++u) j[u] = jn[u];
            if (k + 2 * NL_BATCH <= n) {
#pragma unroll
               for (int u = 0; u < NL_BATCH; ++u) jn[u] = row[(size_t)(k + NL_BATCH + u) * step];
            }
            real_t dx[NL_BATCH], dy[NL_BATCH], dz[NL_BATCH];
#pragma unroll
            for (int u = 0; u < NL_BATCH; ++u) { dx[u] = xi - sp[j[u]]; dy[u] = yi - sp[j[u] + 1]; dz[u] = zi - sp[j[u] + 2]; }
#pragma unroll
            for (int u = 0; u < NL_BATCH; ++u) {
               const real_t r2 = dx[u]*dx[u] + dy[u]*dy[u] + dz[u]*dz[u];
               if (r2 <= a.rc2) ljTablePair<ENERGY>(dx[u], dy[u], dz[u], r2, t, fx, fy, fz, e);
            }
         }
         for (; k < n; ++k) {
            const int j = row[(size_t)k * step];
            const real_t dx = xi - sp[j], dy = yi - sp[j + 1], dz = zi - sp[j + 2];
            const real_t r2 = dx*dx + dy*dy + dz*dz;
            if (r2 <= a.rc2) ljTablePair<ENERGY>(dx, dy, dz, r2, t, fx, fy, fz, e);
         }
      }
   }
   if (G > 1) {                                               // (wave-uniform) all lanes take part; lanes < m keep the sum of the replicas
      if (!active) { fx = fy = fz = e = R(0.0); }
      real_t tx = fx, ty = fy, tz = fz, te = e;
      for (int r = 1; r < G; ++r) {
         const int src = (ai + r * m) & 63;
         tx += bpermuteR(fx, src); ty += bpermuteR(fy, src); tz += bpermuteR(fz, src);
         if (ENERGY) te += bpermuteR(e, src);
      }
      fx = tx; fy = ty; fz = tz; e = te;
   }
   if (active && g == 0) {
      a.fx[iSlot] = fx; a.fy[iSlot] = fy; a.fz[iSlot] = fz;
      if (ENERGY) a.e[iSlot] = e;
   }
}

// ---------------------------------------------------------------------------------------------------
// LJ_Force_thread_atom_nl with the table pair: thread per slot over the global-slot Verlet lists (slabFormat 0: COMD_NL_GLOBAL=1, and cells of
// more than 512 slots, which small boxes have: cells of cutoff + skin in a box of under four of them per axis)
template <bool ENERGY>
__global__ __launch_bounds__(256)
void LJ_Force_thread_atom_nl_table(LjArgs a, NlView nl, TableView t)
{
   int iBox, i;
   if (!nlSlot(a.cells, a.nAtoms, a.nCells, a.cap, iBox, i)) return;
   const size_t iSlot = (size_t)iBox * a.cap + i;
   const real_t xi = a.rx[iSlot], yi = a.ry[iSlot], zi = a.rz[iSlot];
   const int n = nl.count[iSlot];
   const int* __restrict__ row = nl.list + (size_t)iBox * nl.maxNbr * a.cap + i;
   real_t fx = R(0.0), fy = R(0.0), fz = R(0.0), e = R(0.0);
   int k = 0;
   for (; k + 4 <= n; k += 4) {                 // four gathers in flight
      int j[4]; real_t dx[4], dy[4], dz[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) j[u] = row[(size_t)(k + u) * a.cap];
#pragma unroll
      for (int u = 0; u < 4; ++u) { dx[u] = xi - a.rx[j[u]]; dy[u] = yi - a.ry[j[u]]; dz[u] = zi - a.rz[j[u]]; }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
         const real_t r2 = dx[u]*dx[u] + dy[u]*dy[u] + dz[u]*dz[u];
         if (r2 <= a.rc2) ljTablePair<ENERGY>(dx[u], dy[u], dz[u], r2, t, fx, fy, fz, e);
      }
   }
   for (; k < n; ++k) {
      const int j = row[(size_t)k * a.cap];
      const real_t dx = xi - a.rx[j], dy = yi - a.ry[j], dz = zi - a.rz[j];
      const real_t r2 = dx*dx + dy*dy + dz*dz;
      if (r2 <= a.rc2) ljTablePair<ENERGY>(dx, dy, dz, r2, t, fx, fy, fz, e);
   }
   a.fx[iSlot] = fx; a.fy[iSlot] = fy; a.fz[iSlot] = fz;
   if (ENERGY) a.e[iSlot] = e;
}
