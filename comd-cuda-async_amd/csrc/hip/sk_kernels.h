// sk_kernels.h -- the static structure factor on a grid of wave vectors (computeStructureFactor, comd_hip.h): the density amplitudes
//   rho(h, k, l) = sum_j exp(-i K . r_j),   K = 2 pi (sx h / Lx, sy k / Ly, sz l / Lz),   h in [0, M], k, l in [-M, M],
// of THIS rank's local atoms, stored as (M + 1, 2M + 1, 2M + 1) complex doubles.  The reference has no counterpart.  The only analysis here that is no stencil
// walk: N atoms x K vectors of dense arithmetic.
//
// The sum is separable per atom: exp(-i K . r) = ex[h] ey[k] ez[l].  Per atom and axis the fractional coordinate u = (double)r_a / L_a is taken in double in both
// builds; the phase of index m is 2 pi frac((s_a m) u), the integer product s_a m exact, evaluated with sincospi and stored as real_t.  So a position outside
// [0, L) (the *_nl methods between two list builds) needs no wrap: the result is periodic in the box to the rounding of (s m) u.
//
//   SK_amplitudes  grid (tiles, chunks), 256 threads.  The work items are flattened: item i = (pair p, l-block b), i = p nLB + b, p = h (2M + 1) + (k + M); the
//                  l-blocks are SK_LB wide and anchored at 0 (block b starts at l = (b - ceil(M / SK_LB)) SK_LB), so that l = 0 always starts a block.  A tile is
//                  256 consecutive items, a chunk a contiguous range of local cells.  The workgroup walks the occupied slots of its cells in batches of 64
//                  atoms (32 where the tables of 64 would take more than SK_LDS_FOR_64 bytes of LDS); the positions of the next batch are loaded under
//                  the work on the current one.  The threads below the batch size put u into LDS, a barrier, then all threads fill the batch's phase
//                  tables -- per atom ex[h] for the h of the tile, ey[|k|] for the |k| of the tile (ey[-k] is the conjugate), ez at the start of every l-block and ez1 = ez[1] -- a barrier, and
//                  every thread adds the batch to its SK_LB complex accumulators: q = ex[h] ey[k] ez[l0], then SK_LB times acc[j] += q; q *= ez1.  The rotation
//                  never runs longer than SK_LB - 1 steps.  In the float build the real_t accumulators of a batch are added into doubles after every batch, so no
//                  real_t sum is longer than 64 terms.  At the end the item's amplitudes go as doubles into partial[chunk][K][2].
//   SK_sum         adds the chunks' rows in ascending order of the chunk.
// No floating-point atomics: one configuration (method, cell numbering, ranks, chunk count) gives the same bits at every call.  Another atom order gives another
// rounding: the result is NOT the same bits across methods, cell numberings, chunk counts or rank counts.
//
// rho(0, 0, 0): h = k = 0 give ex = ey = (1, -0) and l = 0 starts a block with ez = (1, -0), so every atom adds exactly 1 and the amplitude is N exactly.
//
// Error against the exact sum, per component: N eps(real_t) (16 + 2 pi Hmax) with Hmax the largest |s m| -- the two roundings of u and of (s m) u move a phase by
// at most 2 pi Hmax eps(double) (nothing in the float build, whose eps is eps(float)); the rest is the rounding of the table, two complex products, at most
// SK_LB - 1 rotations and the sum.
//
// The kernels read r and nAtoms and write nothing but their own buffer.
#pragma once
#include "device_common.h"

#define SK_LB 8            // l indices per thread: 2 * SK_LB accumulators in registers
#define SK_BATCH_MAX 64    // atoms whose tables are in LDS at a time: 64, or 32 where 64 would take more than SK_LDS_FOR_64 bytes
#define SK_LDS_FOR_64 32768
#define SK_MAX_M 64
#define SK_MAX_HM 65536    // stride * M at most: the phase index times u keeps 36 bits of the fraction in double

struct SkArgs {
   const real_t* __restrict__ rx; const real_t* __restrict__ ry; const real_t* __restrict__ rz;
   const int* __restrict__ nAtoms;
   int nLocalBoxes, cap, cellsPerChunk, batch;
   int M, W, nLB, lbNeg;      // W = 2M + 1; nLB l-blocks, lbNeg of them below l = 0
   int nItems;                // (M + 1) W nLB
   int sx, sy, sz;
   double Lx, Ly, Lz;
   double* __restrict__ partial;      // [chunks][K][2], K = (M + 1) W W
};

// the part of the tables one tile needs: h in [hLo, hLo + nH), |k| in [kaLo, kaLo + nKa); T = nH + nKa + nLB + 1 entries per atom.  Host and device share it:
// the host sizes the LDS with the largest T over the tiles
struct SkTile { int hLo, nH, kaLo, nKa; };
__host__ __device__ inline SkTile skTileOf(int tile, int nItems, int nLB, int W, int M)
{
   const int first = tile * 256, last = (first + 255 < nItems ? first + 255 : nItems - 1);
   const int pFirst = first / nLB, pLast = last / nLB;
   SkTile t;
   t.hLo = pFirst / W; t.nH = pLast / W - t.hLo + 1;
   if (t.nH == 1) {
      const int kMin = pFirst % W - M, kMax = pLast % W - M;      // kMin <= kMax
      const int aMin = kMin < 0 ? -kMin : kMin, aMax = kMax < 0 ? -kMax : kMax;
      t.kaLo = (kMin <= 0 && kMax >= 0) ? 0 : (aMin < aMax ? aMin : aMax);
      t.nKa = (aMin > aMax ? aMin : aMax) - t.kaLo + 1;
   } else { t.kaLo = 0; t.nKa = M + 1; }
   return t;
}

// exp(-2 pi i frac(n u)) in the build's precision
__device__ __forceinline__ real2 skPhase(int n, double u)
{
   const double x = (double)n * u;
   const double t = x - __builtin_floor(x);      // [0, 1]
   double s, c;
   sincospi(2.0 * t, &s, &c);
   real2 e; e.x = (real_t)c; e.y = (real_t)(-s);
   return e;
}

__device__ __forceinline__ real2 skMul(real2 a, real2 b)
{
   real2 c;
   c.x = a.x * b.x - a.y * b.y;
   c.y = a.x * b.y + a.y * b.x;
   return c;
}

__global__ __launch_bounds__(256)
void SK_amplitudes(SkArgs v)
{
   extern __shared__ double sSk[];              // [batch][3] u, then [batch][T] real2
   double* __restrict__ sU = sSk;
   real2* __restrict__ sTab = reinterpret_cast<real2*>(sSk + 3 * v.batch);
   const int t = (int)threadIdx.x;
   const SkTile tile = skTileOf((int)blockIdx.x, v.nItems, v.nLB, v.W, v.M);
   const int T = tile.nH + tile.nKa + v.nLB + 1;

   // this thread's item
   const int item = (int)blockIdx.x * 256 + t;
   const bool live = item < v.nItems;
   const int p = live ? item / v.nLB : 0, b = live ? item % v.nLB : 0;
   const int h = p / v.W, k = p % v.W - v.M;
   const int l0 = (b - v.lbNeg) * SK_LB;
   const int iX = h - tile.hLo, iY = tile.nH + (k < 0 ? -k : k) - tile.kaLo, iZ = tile.nH + tile.nKa + b, iZ1 = T - 1;
   const real_t conjY = k < 0 ? R(-1.0) : R(1.0);

   real_t accR[SK_LB], accI[SK_LB];
#ifdef COMD_SINGLE
   double sumR[SK_LB], sumI[SK_LB];
#pragma unroll
   for (int j = 0; j < SK_LB; ++j) sumR[j] = sumI[j] = 0.0;
#endif
#pragma unroll
   for (int j = 0; j < SK_LB; ++j) accR[j] = accI[j] = R(0.0);

   const int cellEnd = min(((int)blockIdx.y + 1) * v.cellsPerChunk, v.nLocalBoxes);
   int cell = (int)blockIdx.y * v.cellsPerChunk, s = 0;      // the next slot to take: uniform over the workgroup
   // the next batch: up to v.batch occupied slots, over as many cells as it takes; thread t < n gets the slot of the batch's atom t.  Returns n, 0 at the end
   auto nextBatch = [&](long& slot) {
      int n = 0;
      slot = -1;
      while (n < v.batch && cell < cellEnd) {
         const int inCell = min(v.nAtoms[cell], v.cap);
         const int take = min(v.batch - n, inCell - s);
         if (take > 0) {
            if (t >= n && t < n + take) slot = (long)cell * v.cap + s + (t - n);
            n += take; s += take;
         }
         if (s >= inCell) { ++cell; s = 0; }
      }
      return n;
   };
   long slot;
   int nB = nextBatch(slot);
   real_t rx = R(0.0), ry = R(0.0), rz = R(0.0);
   if (slot >= 0) { rx = v.rx[slot]; ry = v.ry[slot]; rz = v.rz[slot]; }
   while (nB > 0) {
      __syncthreads();            // the tables of the batch before are read
      if (t < nB) {
         sU[3 * t] = (double)rx / v.Lx;
         sU[3 * t + 1] = (double)ry / v.Ly;
         sU[3 * t + 2] = (double)rz / v.Lz;
      }
      __syncthreads();
      // the positions of the batch after this one travel while this one is worked on
      const int nNext = nextBatch(slot);
      if (slot >= 0) { rx = v.rx[slot]; ry = v.ry[slot]; rz = v.rz[slot]; }
      for (int e = t; e < nB * T; e += 256) {
         const int a = e / T, i = e - a * T;
         int n; double u;
         if (i < tile.nH) { n = v.sx * (tile.hLo + i); u = sU[3 * a]; }
         else if (i < tile.nH + tile.nKa) { n = v.sy * (tile.kaLo + i - tile.nH); u = sU[3 * a + 1]; }
         else if (i < T - 1) { n = v.sz * ((i - tile.nH - tile.nKa - v.lbNeg) * SK_LB); u = sU[3 * a + 2]; }
         else { n = v.sz; u = sU[3 * a + 2]; }
         sTab[e] = skPhase(n, u);
      }
      __syncthreads();
      if (live) {
         for (int a = 0; a < nB; ++a) {
            const real2* __restrict__ row = sTab + a * T;
            real2 ey = row[iY]; ey.y *= conjY;
            real2 q = skMul(skMul(row[iX], ey), row[iZ]);
            const real2 ez1 = row[iZ1];
#pragma unroll
            for (int j = 0; j < SK_LB; ++j) {
               accR[j] += q.x; accI[j] += q.y;
               if (j + 1 < SK_LB) q = skMul(q, ez1);
            }
         }
#ifdef COMD_SINGLE
#pragma unroll
         for (int j = 0; j < SK_LB; ++j) { sumR[j] += (double)accR[j]; sumI[j] += (double)accI[j]; accR[j] = accI[j] = 0.0f; }
#endif
      }
      nB = nNext;
   }

   if (live) {
      const size_t K = (size_t)(v.M + 1) * v.W * v.W;
      double* __restrict__ out = v.partial + ((size_t)blockIdx.y * K + (size_t)p * v.W) * 2;
#pragma unroll
      for (int j = 0; j < SK_LB; ++j) {
         const int l = l0 + j;
         if (l >= -v.M && l <= v.M) {
#ifdef COMD_SINGLE
            out[2 * (l + v.M)] = sumR[j]; out[2 * (l + v.M) + 1] = sumI[j];
#else
            out[2 * (l + v.M)] = accR[j]; out[2 * (l + v.M) + 1] = accI[j];
#endif
         }
      }
   }
}

// out[i] = partial[0][i] + partial[1][i] + ... in that order, i < n = 2 K
__global__ __launch_bounds__(256)
void SK_sum(const double* __restrict__ partial, int nChunks, size_t n, double* __restrict__ out)
{
   const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   double sum = partial[i];
   for (int c = 1; c < nChunks; ++c) sum += partial[(size_t)c * n + i];
   out[i] = sum;
}
