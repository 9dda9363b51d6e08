// born_kernels.h -- the Born matrix for gfx950 (computeBornMatrix, comd_hip.h).  The reference has no counterpart.
//
//   B_abcd = d^2 U / d eta_ab d eta_cd at the current configuration, eta the Lagrangian strain, in eV (extensive):
//   B_abcd = sum_i [ sum_j ( 1/2 (phi'' - phi'/r) + F'_i (rho'' - rho'/r) ) r_a r_b r_c r_d / r^2  +  F''(rhobar_i) g^i_ab g^i_cd ]
//   g^i_ab = sum_j rho'(r) r_a r_b / r
// j over the neighbours (local or halo image) with 0 < r^2 <= rc^2: the acceptance test of virial_kernels.h, every pair seen from both sides.  The
// embedding part of a pair is split as F'_i per side, so no dfEmbed of a halo slot is read.  Voigt order xx yy zz yz xz xy; the output is the upper
// triangle of the 6 x 6 matrix, row-major: 21 numbers.
//
// The derivatives are those of the force the kernels apply, one sibling functor per pair function of virial_kernels.h:
//   BornLj           analytic: 1/2 (phi'' - phi'/r) / r^2 = 24 eps s6 r^-10 (14 s6 r^-6 - 4); the constant factor once per lane, as LJ_FORCE_SCALE
//   BornLjTable      the -I table: interpolate's df = (g1 + u (g2 - g1)) invDxHalf, and its derivative (g2 - g1) invDxHalf invDx, constant on the
//   BornEam<false>   segment interpolate lands on (clamped arguments included): tableDerivatives below, the index arithmetic of interpolate<true>
//   BornEam<true>    -P, cubic in x = r^2: phi'' - phi'/r = 4 r^2 f''(x), f''(x) = 6 a x + 2 b on interpolateSpline's interval; rho'/r = 2 f'(x)
// F'_i is dfEmbed[i] and F''_i the derivative of the quadratic F table on the segment of rhobar[i]: both of the last force evaluation (computeVirial's contract).
//
// Mapping: the chunk walk of stencil_walk.h, lane = atom i.  The pair part is fully symmetric in abcd: 15 sums r_a r_b r_c r_d k, which are the first 15
// entries of the upper triangle (rows xx, yy, zz); the other six (yz yz, yz xz, yz xy, xz xz, xz xy, xy xy) repeat yyzz, xyzz, xyyz, xxzz, xxyz, xxyy.
// Within a chunk each lane adds its pairs' 15 terms and the six g of its atom in real_t.  A replicated chunk (reps > 1) adds g over the copies first
// (sumOverCopies), and copy 0 alone forms F'' g (x) g.  Inactive lanes add nothing.
// Reduction: at the end of the chunk the 15 + 21 lane values are converted to double and added over the wave (the butterfly of blockSumD, every lane ends with
// the same bits), and lane c < 21 adds entry c of the triangle -- scale() x its pair sum + its embedding product -- into the one double it keeps over the
// chunks of the wave.  The sums are chunk-local on purpose: accumulators carried over the chunks through both paths of stencilWalk were held twice by the
// register allocator (191 VGPRs for the EAM instances of the double build), and 21 embedding accumulators per lane cost 42 more; this way a lane carries
// two VGPRs from chunk to chunk, at the price of 36 wave sums per chunk.  blockSumD then adds the four waves in a fixed order into one row of 21 per
// workgroup, and BornMatrix_Final adds the rows in a fixed order.  No atomics, no LDS beyond blockSumD's, no scratch; bit-reproducible.  The kernels read
// r, rhobar, dfEmbed, the tables and the cell tables and write nothing but their rows.
#pragma once
#include "virial_kernels.h"

#define BORN_N 21                      // the upper triangle of the 6 x 6 matrix
#define BORN_PAIR_N 15                 // the fully symmetric sums: the entries of the rows xx, yy, zz
#define BORN_BLOCKS 2048               // rows of partials: fixed, so the order of the sums does not depend on the system

struct BornArgs : StencilArgs {
   real_t rc2;
};

// df/dr and d2f/dr2 of the quadratic table: interpolate<true>'s segment and df, and the derivative of that df
__device__ __forceinline__ void tableDerivatives(const TableView& t, real_t r, real_t& df, real_t& d2f)
{
   r = maxR(r, t.x0); r = minR(r, t.xn);
   r = r * t.invDx - t.invDxXx0;
   const real_t ri = floorR(r);
   const int ii = (int)ri;
   r -= ri;
   const real_t v0 = t.v[ii], v1 = t.v[ii + 1], v2 = t.v[ii + 2], v3 = t.v[ii + 3];
   const real_t g1 = v2 - v0, g2 = v3 - v1, gg = (g2 - g1) * t.invDxHalf;
   df = fmaR(r, gg, g1 * t.invDxHalf);
   d2f = gg * t.invDx;
}

// f'(x) and f''(x) of the -P spline in x = r^2, on interpolateSpline's interval
__device__ __forceinline__ void splineDerivatives(const InterpolationSplineObjectGpu& t, real_t r2, real_t& df, real_t& d2f)
{
   float r = __builtin_sqrtf((float)r2);
   r = fmaxf(r, t.x0);
   r = fminf(r, t.xn);
   r = r * t.invDx - t.invDxXx0;
   int ii = (int)floorf(r);
   ii = ii < t.n - 1 ? ii : t.n - 1;
   const real_t* __restrict__ c = t.coefficients + 4 * ii;
   const real_t a = c[0], b = c[1], cc = c[2];
   df = (R(3.0) * a * r2 + R(2.0) * b) * r2 + cc;
   d2f = R(6.0) * a * r2 + R(2.0) * b;
}

// The pair functors: begin(iOff) once per i atom, then operator() per accepted pair returns k and h with
//    scale() k r_a r_b r_c r_d  the pair's term of B_abcd on the side of i,   h r_a r_b  its term of g^i_ab (EMBED only);
// d2Embed(): F''(rhobar_i) (EMBED only)
struct BornLj {
   real_t s6x14, fs;
   static constexpr bool EMBED = false;
   __host__ __device__ real_t scale() const { return fs; }
   __device__ void begin(size_t) {}
   __device__ real_t d2Embed() const { return R(0.0); }
   __device__ void operator()(real_t r2, real_t& k, real_t& h) const
   {
      const real_t ir2 = rcpR(r2);
      const real_t t = ir2 * ir2;
      const real_t w = t * ir2;
      k = (t * w) * fmaR(w, s6x14, -R(4.0));
      h = R(0.0);
   }
};

struct BornLjTable {
   TableView t;
   static constexpr bool EMBED = false;
   __host__ __device__ real_t scale() const { return R(1.0); }
   __device__ void begin(size_t) {}
   __device__ real_t d2Embed() const { return R(0.0); }
   __device__ void operator()(real_t r2, real_t& k, real_t& h) const
   {
      const real_t y = rsqrtR(r2);
      real_t dv, d2v;
      tableDerivatives(t, r2 * y, dv, d2v);
      k = R(0.5) * fmaR(-dv, y, d2v) * (y * y);
      h = R(0.0);
   }
};

template <bool SPLINE>
struct BornEam {
   InterpolationObjectGpu phi, rho, f;
   InterpolationSplineObjectGpu phiS, rhoS;
   const real_t* __restrict__ dfEmbed;
   const real_t* __restrict__ rhobar;
   real_t dfi, d2fi;
   static constexpr bool EMBED = true;
   __host__ __device__ real_t scale() const { return R(1.0); }
   __device__ void begin(size_t iOff)
   {
      real_t dF;
      dfi = dfEmbed[iOff];
      tableDerivatives(makeTable(f, f.values), rhobar[iOff], dF, d2fi);
   }
   __device__ real_t d2Embed() const { return d2fi; }
   __device__ void operator()(real_t r2, real_t& k, real_t& h) const
   {
      if (SPLINE) {
         real_t dphi, d2phi, drho, d2rho;
         splineDerivatives(phiS, r2, dphi, d2phi);
         splineDerivatives(rhoS, r2, drho, d2rho);
         k = fmaR(R(4.0) * dfi, d2rho, R(2.0) * d2phi);
         h = R(2.0) * drho;
      } else {
         const real_t y = rsqrtR(r2), r = r2 * y;
         real_t dphi, d2phi, drho, d2rho;
         tableDerivatives(makeTable(phi, phi.values), r, dphi, d2phi);
         k = R(0.5) * fmaR(-dphi, y, d2phi);
         __builtin_amdgcn_sched_barrier(0);
         tableDerivatives(makeTable(rho, rho.values), r, drho, d2rho);
         h = drho * y;
         k = fmaR(dfi, d2rho - h, k) * (y * y);
      }
   }
};

// t[0..N) -> their sums over the 64 lanes, every lane ends with them (m = 32 ... 1, a + b is what both lanes of a pair compute: the order of blockSumD)
template <int N>
__device__ __forceinline__ void waveSumsD(double (&t)[N], int lane)
{
#pragma unroll
   for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
      for (int c = 0; c < N; ++c) t[c] += bpermuteR(t[c], lane ^ m);
}

// partial: [gridDim.x][BORN_N].  A kernel parameter of its own, __restrict__, not a member of the argument record: see stress_kernels.h
template <class PAIR>
__global__ __launch_bounds__(256)
void BornMatrix_thread_atom(BornArgs v, PAIR pair, double* __restrict__ partial)
{
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;
   // the six entries below the rows xx, yy, zz repeat a pair sum: yz yz = yyzz (7), yz xz = xyzz (14), yz xy = xyyz (9), xz xz = xxzz (2), xz xy = xxyz (3),
   // xy xy = xxyy (1): twin[c] is the second lane pair sum c goes to
   constexpr int twin[BORN_PAIR_N] = { -1, 20, 18, 19, -1, -1, -1, 15, -1, 17, -1, -1, -1, -1, 16 };
   const double fs = (double)pair.scale();
   double total = 0.0;                 // lane c < 21: entry c of the triangle, over the chunks of the wave

   forEachChunk(v, lane, wave, [&](int iBox, int first, int, int reps, int span, int q, int ia, bool active) {
      const size_t iOff = (size_t)iBox * v.cap + (active ? ia : first);
      const real_t xi = v.rx[iOff], yi = v.ry[iOff], zi = v.rz[iOff];
      pair.begin(iOff);
      real_t acc[BORN_PAIR_N], g[6];
#pragma unroll
      for (int c = 0; c < BORN_PAIR_N; ++c) acc[c] = R(0.0);
#pragma unroll
      for (int c = 0; c < 6; ++c) g[c] = R(0.0);
      auto test = [&](real_t xj, real_t yj, real_t zj, size_t) {
         const real_t dx = xi - xj, dy = yi - yj, dz = zi - zj;
         const real_t r2 = dx*dx + dy*dy + dz*dz;
         if (active && r2 <= v.rc2 && r2 > R(0.0)) {
            real_t k, h;
            pair(r2, k, h);
            const real_t xx = dx * dx, yy = dy * dy, zz = dz * dz, yz = dy * dz, xz = dx * dz, xy = dx * dy;
            const real_t kxx = k * xx, kyy = k * yy, kzz = k * zz;
            acc[0]  = fmaR(kxx, xx, acc[0]);  acc[1]  = fmaR(kxx, yy, acc[1]);  acc[2]  = fmaR(kxx, zz, acc[2]);
            acc[3]  = fmaR(kxx, yz, acc[3]);  acc[4]  = fmaR(kxx, xz, acc[4]);  acc[5]  = fmaR(kxx, xy, acc[5]);
            acc[6]  = fmaR(kyy, yy, acc[6]);  acc[7]  = fmaR(kyy, zz, acc[7]);  acc[8]  = fmaR(kyy, yz, acc[8]);
            acc[9]  = fmaR(kyy, xz, acc[9]);  acc[10] = fmaR(kyy, xy, acc[10]);
            acc[11] = fmaR(kzz, zz, acc[11]); acc[12] = fmaR(kzz, yz, acc[12]); acc[13] = fmaR(kzz, xz, acc[13]);
            acc[14] = fmaR(kzz, xy, acc[14]);
            if (PAIR::EMBED) {
               g[0] = fmaR(h, xx, g[0]); g[1] = fmaR(h, yy, g[1]); g[2] = fmaR(h, zz, g[2]);
               g[3] = fmaR(h, yz, g[3]); g[4] = fmaR(h, xz, g[4]); g[5] = fmaR(h, xy, g[5]);
            }
         }
      };
      stencilWalk<size_t>(v, iBox, reps, q, test);
      // the chunk's sums over the wave, five at a time (all at once would hold 2 x 15 doubles in flight); lane c keeps entry c
#pragma unroll
      for (int c0 = 0; c0 < BORN_PAIR_N; c0 += 5) {
         double t[5];
#pragma unroll
         for (int u = 0; u < 5; ++u) t[u] = (double)acc[c0 + u];
         waveSumsD(t, lane);
#pragma unroll
         for (int u = 0; u < 5; ++u) if (lane == c0 + u || lane == twin[c0 + u]) total = __builtin_fma(fs, t[u], total);
         __builtin_amdgcn_sched_barrier(0);
      }
      if (PAIR::EMBED) {
         if (reps > 1) sumOverCopies(lane, span, g[0], g[1], g[2], g[3], g[4], g[5]);
         const real_t d2 = active && q == 0 ? pair.d2Embed() : R(0.0);
         int c = 0;
#pragma unroll
         for (int a = 0; a < 6; ++a) {         // a row of the triangle at a time
            const real_t ga = d2 * g[a];
            double t[6];
#pragma unroll
            for (int b = 0; b < 6; ++b) t[b] = b >= a ? (double)(ga * g[b]) : 0.0;
            waveSumsD(t, lane);
#pragma unroll
            for (int b = a; b < 6; ++b, ++c) if (lane == c) total += t[b];
            __builtin_amdgcn_sched_barrier(0);
         }
      }
   });
   double sum[BORN_N];
#pragma unroll
   for (int c = 0; c < BORN_N; ++c) sum[c] = lane == c ? total : 0.0;
   blockSumD(sum, partial + (size_t)blockIdx.x * BORN_N);
}

// the rows of partials -> out[BORN_N], in a fixed order
__global__ __launch_bounds__(256)
void BornMatrix_Final(const double* __restrict__ partial, int nPartial, double* __restrict__ out)
{
   double acc[BORN_N];
#pragma unroll
   for (int c = 0; c < BORN_N; ++c) acc[c] = 0.0;
   for (int i = threadIdx.x; i < nPartial; i += blockDim.x)
#pragma unroll
      for (int c = 0; c < BORN_N; ++c) acc[c] += partial[(size_t)i * BORN_N + c];
   blockSumD(acc, out);
}
