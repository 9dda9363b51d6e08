// steinhardt_kernels.h -- per-atom bond-orientational order for gfx950: Steinhardt's q4, q6, w4, w6 (computeSteinhardt, computeSteinhardtSummary,
// comd_hip.h; Steinhardt, Nelson, Ronchetti 1983).  The reference has no counterpart.
//
// For every local atom i, with its 12 nearest neighbours j != i (local or halo image) inside the force cutoff -- the set, the tie rule and the walk of
// nearest12_walk.h, as the centro-symmetry parameter (csp_kernels.h) -- and the unit vectors u_ij = (r_j - r_i) / |r_j - r_i|:
//   q_lm(i) = 1/12 sum_j Y_lm(u_ij)                      l = 4 and 6
//   q_l     = sqrt( 4 pi / (2l + 1) sum_m |q_lm|^2 )
//   w_l     = sum_{m1 + m2 + m3 = 0} (l l l; m1 m2 m3) q_lm1 q_lm2 q_lm3 / (sum_m |q_lm|^2)^(3/2)         the normalised third-order invariant
// w_l is 0 where q_l^2 < 1e-6 (the icosahedron's w4 is 0/0).  An atom with fewer than 12 neighbours inside the cutoff is invalid: all four are NaN.
//
// The harmonics: Y_lm(u) = (-1)^m sqrt((2l + 1)/(4 pi) (l - m)!/(l + m)!) (x + iy)^m d^m P_l(z)/dz^m for m >= 0, and q_l,-m = (-1)^m conj(q_lm), so the
// stage keeps only A_lm = sum_j (x + iy)^m P_l^(m)(z), m = 0..l: 9 + 13 real sums, added in the ascending-r^2 order of d[] / id[], the powers of x + iy by
// a recurrence and the derivatives of the Legendre polynomials as polynomials in z.  With a_lm = (-1)^m sqrt((l - m)!/(l + m)!) A_lm,
// S_l = a_l0^2 + 2 sum_{m>0} |a_lm|^2:  q_l^2 = S_l / 144, and w_l = W_l / S_l^(3/2) with W_l the triple sum over the a_lm (the common factors cancel).
// The triple sum: the 3j symbol of three equal even l is symmetric under every permutation of its columns and under m -> -m, which turns the product of the
// three q into its conjugate.  So W_l = sum over the sets {m1 >= m2 > 0, -(m1 + m2)} of 2 perms (3j) Re(a_m1 a_m2 conj a_(m1+m2)) (-1)^(m1+m2), perms = 3 for
// m1 = m2 and 6 otherwise, plus the sets {m, 0, -m}: (3j) a_0^3 for m = 0 and 6 (3j) (-1)^m a_0 |a_m|^2 for m > 0.  4 + 5 terms for l = 4, 9 + 7 for l = 6.
// The 3j symbols are compile-time constants of the Racah formula (wigner3jEqualL below).
//
// Mapping: the chunk walk of stencil_walk.h; selection and merge are the text of nearest12_walk.h, replicated small chunks included.  As in the csp kernel the
// last stage runs on copy 0 alone.  It reads the 12 positions again by slot.  Every index is a compile-time one: no scratch.  No atomics, no LDS.
// Output: four SoA planes [4][nLocalBoxes*cap] of real_t, q4 q6 w4 w6.  The kernel reads r, nAtoms and nbr and writes nothing but its planes.
//
// Steinhardt_Summary / Steinhardt_SummaryFinal (slot_summary.h): the valid and the invalid atoms (a NaN in the q4 plane; they stay out of sums and extremes),
// sum q4, q6, w4, w6 in double, min q6 with the gid that holds it (ties: the lowest gid), max q6, the atoms with q6 >= the threshold.
#pragma once
#include <utility>
#include "csp_kernels.h"
#include "slot_summary.h"

#define STEINHARDT_BLOCKS 2048         // the grid of the walk, as CSP_BLOCKS
#define STEINHARDT_SUM_BLOCKS 512      // rows of the summary: fixed, so the order of the sums does not depend on the system
#define STEINHARDT_SUM_N 10            // valid, invalid, sum q4, sum q6, sum w4, sum w6, min q6, its gid, max q6, atoms at or above the threshold
#define STEINHARDT_PLANES 4            // q4 q6 w4 w6

struct SteinhardtArgs : StencilArgs {
   real_t rc2;                        // cutoff^2
   size_t plane;                      // nLocalBoxes * cap: the slots of one plane of the output
};

constexpr double stFactorial(int n) { double f = 1.0; for (int k = 2; k <= n; ++k) f *= (double)k; return f; }
constexpr double stSqrt(double x)
{
   if (!(x > 0.0)) return 0.0;
   double y = x > 1.0 ? x : 1.0;
   for (int k = 0; k < 200; ++k) y = 0.5 * (y + x / y);      // Newton from above: monotone, at round-off long before the last step
   return y;
}

// (l l l; m1 m2 m3), m1 + m2 + m3 = 0, by the Racah formula
//   (-1)^(-m3) sqrt( l!^3 / (3l + 1)!  prod_i (l + m_i)! (l - m_i)! )  sum_t (-1)^t / ( t! (t + m1)! (t - m2)! (l - t)! (l - t - m1)! (l - t + m2)! )
// over the t that keep every factorial's argument >= 0
constexpr double wigner3jEqualL(int l, int m1, int m2, int m3)
{
   if (m1 + m2 + m3 != 0) return 0.0;
   double sum = 0.0;
   for (int t = 0; t <= l; ++t) {
      if (t + m1 < 0 || t - m2 < 0 || l - t - m1 < 0 || l - t + m2 < 0) continue;
      const double den = stFactorial(t) * stFactorial(t + m1) * stFactorial(t - m2) * stFactorial(l - t) * stFactorial(l - t - m1) * stFactorial(l - t + m2);
      sum += ((t & 1) ? -1.0 : 1.0) / den;
   }
   const double delta = stFactorial(l) * stFactorial(l) * stFactorial(l) / stFactorial(3 * l + 1);
   const double prod = stFactorial(l + m1) * stFactorial(l - m1) * stFactorial(l + m2) * stFactorial(l - m2) * stFactorial(l + m3) * stFactorial(l - m3);
   return ((m3 & 1) ? -1.0 : 1.0) * stSqrt(delta * prod) * sum;
}

// (-1)^m sqrt((l - m)! / (l + m)!): A_lm -> a_lm
constexpr double stScale(int l, int m) { return ((m & 1) ? -1.0 : 1.0) * stSqrt(stFactorial(l - m) / stFactorial(l + m)); }

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a constant expression in the body
template <class F, int... I>
__device__ __forceinline__ void stStaticForSeq(std::integer_sequence<int, I...>, F f) { (f(std::integral_constant<int, I>()), ...); }
template <int N, class F>
__device__ __forceinline__ void stStaticFor(F f) { stStaticForSeq(std::make_integer_sequence<int, N>(), f); }

// from the sums A_lm = re[m] + i im[m]: q_l^2 and w_l (0 where q_l^2 < 1e-6)
template <int L>
__device__ __forceinline__ void stInvariants(const real_t (&re)[L + 1], const real_t (&im)[L + 1], real_t& q2, real_t& w)
{
   real_t a[L + 1], b[L + 1];          // a_lm = a + i b
   stStaticFor<L + 1>([&](auto mc) {
      constexpr int m = decltype(mc)::value;
      constexpr real_t s = (real_t)stScale(L, m);
      a[m] = s * re[m]; b[m] = s * im[m];
   });
   real_t S = R(0.0), W = R(0.0);
   stStaticFor<L>([&](auto mc) {          // the sets {m, 0, -m}, m = L ... 1: the small terms first
      constexpr int m = L - decltype(mc)::value;
      constexpr real_t t = (real_t)(6.0 * ((m & 1) ? -1.0 : 1.0) * wigner3jEqualL(L, m, 0, -m));
      const real_t n2 = a[m] * a[m] + b[m] * b[m];
      S += n2; W += t * n2;
   });
   S = a[0] * a[0] + R(2.0) * S;
   constexpr real_t t000 = (real_t)wigner3jEqualL(L, 0, 0, 0);
   W = a[0] * (W + t000 * (a[0] * a[0]));
   stStaticFor<L / 2>([&](auto m2c) {     // the sets {m1 >= m2 > 0, -(m1 + m2)}
      constexpr int m2 = decltype(m2c)::value + 1;
      stStaticFor<L - 2 * m2 + 1>([&](auto m1c) {
         constexpr int m1 = decltype(m1c)::value + m2, m3 = m1 + m2;
         constexpr real_t t = (real_t)(2.0 * (m1 == m2 ? 3.0 : 6.0) * ((m3 & 1) ? -1.0 : 1.0) * wigner3jEqualL(L, m1, m2, -m3));
         const real_t pr = a[m1] * a[m2] - b[m1] * b[m2], pi = a[m1] * b[m2] + b[m1] * a[m2];
         W += t * (pr * a[m3] + pi * b[m3]);
      });
   });
   q2 = S * R(1.0 / 144.0);
   const real_t is = rsqrtR(q2 < R(1e-6) ? R(1.0) : S);
   w = q2 < R(1e-6) ? R(0.0) : W * (is * is * is);
}

// The 12 neighbours' terms do not depend on one another, and left alone the compiler starts them all at once: 36 loads through 36 addresses of 64 bits, and the
// terms side by side as vectors over the neighbours, where the walk has left room for one neighbour's (0.4 to 0.7 kB of scratch in both builds).  An empty asm
// that takes the sums in and out after a neighbour orders them: all of that neighbour's terms are in by then, and the next one's cannot be formed alongside.
// It emits no instruction.  (Two statements: an asm takes 30 operands at most, and an in-out one counts twice.)
#define ST_HOLD9(a, b, c, d, e, f, g, h, i) asm("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h), "+v"(i))
#define ST_HOLD13(a, b, c, d, e, f, g, h, i, j, k, l, m) \
   asm("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h), "+v"(i), "+v"(j), "+v"(k), "+v"(l), "+v"(m))

// out: [4][plane].  A kernel parameter of its own, __restrict__, and not a member of the argument record: see AtomStress_thread_atom (stress_kernels.h),
// which stores inside the loop over the chunks as this kernel does.
__global__ __launch_bounds__(256, 4)
void Steinhardt_thread_atom(SteinhardtArgs v, real_t* __restrict__ out)
{
   const int lane = laneId(), wave = (int)threadIdx.x >> 6;

   forEachChunk(v, lane, wave, [&](int iBox, int first, int, int reps, int span, int q, int ia, bool active) {
#define NN12_COORD(x)
#include "nearest12_walk.h"       // the 12 nearest of the lane's atom: me, xi, yi, zi, d[], id[]
#undef NN12_COORD

      if (active && q == 0) {
         const bool full = id[CSP_NN - 1] >= 0;
         real_t re4[5], im4[5], re6[7], im6[7];
#pragma unroll
         for (int m = 0; m < 5; ++m) { re4[m] = R(0.0); im4[m] = R(0.0); }
#pragma unroll
         for (int m = 0; m < 7; ++m) { re6[m] = R(0.0); im6[m] = R(0.0); }
         const int s0 = full ? id[0] : me;
         real_t xj = v.rx[s0], yj = v.ry[s0], zj = v.rz[s0];
#pragma unroll
         for (int k = 0; k < CSP_NN; ++k) {
            const real_t dx = xj - xi, dy = yj - yi, dz = zj - zi;
            if (k + 1 < CSP_NN) {          // the next neighbour's position is on its way while this one's terms are formed
               const int s = full ? id[k + 1] : me;
               xj = v.rx[s]; yj = v.ry[s]; zj = v.rz[s];
            }
            const real_t r2 = dx*dx + dy*dy + dz*dz;
            const real_t ir = rsqrtR(full ? r2 : R(1.0));
            const real_t x = dx * ir, y = dy * ir, z = dz * ir, z2 = z * z;
            // (x + iy)^m, m = 1..6
            const real_t c1r = x, c1i = y;
            const real_t c2r = x * x - y * y, c2i = R(2.0) * (x * y);
            const real_t c3r = c2r * x - c2i * y, c3i = c2r * y + c2i * x;
            const real_t c4r = c2r * c2r - c2i * c2i, c4i = R(2.0) * (c2r * c2i);
            const real_t c5r = c4r * x - c4i * y, c5i = c4r * y + c4i * x;
            const real_t c6r = c3r * c3r - c3i * c3i, c6i = R(2.0) * (c3r * c3i);
            // d^m P_4 / dz^m
            const real_t p40 = ((R(35.0) * z2 - R(30.0)) * z2 + R(3.0)) * R(0.125);
            const real_t p41 = (R(17.5) * z2 - R(7.5)) * z;
            const real_t p42 = R(52.5) * z2 - R(7.5);
            const real_t p43 = R(105.0) * z;
            // d^m P_6 / dz^m
            const real_t p60 = (((R(231.0) * z2 - R(315.0)) * z2 + R(105.0)) * z2 - R(5.0)) * R(0.0625);
            const real_t p61 = ((R(693.0) * z2 - R(630.0)) * z2 + R(105.0)) * z * R(0.125);
            const real_t p62 = ((R(3465.0) * z2 - R(1890.0)) * z2 + R(105.0)) * R(0.125);
            const real_t p63 = (R(1732.5) * z2 - R(472.5)) * z;
            const real_t p64 = R(5197.5) * z2 - R(472.5);
            const real_t p65 = R(10395.0) * z;
            re4[0] += p40;
            re4[1] += c1r * p41; im4[1] += c1i * p41;
            re4[2] += c2r * p42; im4[2] += c2i * p42;
            re4[3] += c3r * p43; im4[3] += c3i * p43;
            re4[4] += c4r * R(105.0); im4[4] += c4i * R(105.0);
            re6[0] += p60;
            re6[1] += c1r * p61; im6[1] += c1i * p61;
            re6[2] += c2r * p62; im6[2] += c2i * p62;
            re6[3] += c3r * p63; im6[3] += c3i * p63;
            re6[4] += c4r * p64; im6[4] += c4i * p64;
            re6[5] += c5r * p65; im6[5] += c5i * p65;
            re6[6] += c6r * R(10395.0); im6[6] += c6i * R(10395.0);
            ST_HOLD9(re4[0], re4[1], im4[1], re4[2], im4[2], re4[3], im4[3], re4[4], im4[4]);
            ST_HOLD13(re6[0], re6[1], im6[1], re6[2], im6[2], re6[3], im6[3], re6[4], im6[4], re6[5], im6[5], re6[6], im6[6]);
         }
         real_t q42, w4, q62, w6;
         stInvariants<4>(re4, im4, q42, w4);
         stInvariants<6>(re6, im6, q62, w6);
         const real_t nan = R(__builtin_nan(""));
         real_t* __restrict__ o = out + me;
         o[0] = full ? q42 * rsqrtR(q42 > R(0.0) ? q42 : R(1.0)) : nan;
         o[v.plane] = full ? q62 * rsqrtR(q62 > R(0.0) ? q62 : R(1.0)) : nan;
         o[2 * v.plane] = full ? w4 : nan;
         o[3 * v.plane] = full ? w6 : nan;
      }
   });
}

// one candidate of the summary (slot_summary.h): the sums and the counts add, the extremes compare; of two equal minima the lower gid stays
struct SteinhardtSum {
   double sumQ4, sumQ6, sumW4, sumW6, minQ6, maxQ6;
   int gid, n, bad, above;
   static constexpr int N = STEINHARDT_SUM_N;

   __device__ static SteinhardtSum empty() { return SteinhardtSum{ 0.0, 0.0, 0.0, 0.0, __builtin_huge_val(), -__builtin_huge_val(), -1, 0, 0, 0 }; }
   __device__ void join(const SteinhardtSum& b)
   {
      sumQ4 += b.sumQ4; sumQ6 += b.sumQ6; sumW4 += b.sumW4; sumW6 += b.sumW6; n += b.n; bad += b.bad; above += b.above;
      maxQ6 = b.maxQ6 > maxQ6 ? b.maxQ6 : maxQ6;
      const bool take = b.gid >= 0 && (gid < 0 || b.minQ6 < minQ6 || (b.minQ6 == minQ6 && b.gid < gid));
      minQ6 = take ? b.minQ6 : minQ6; gid = take ? b.gid : gid;
   }
   __device__ void toRow(double* __restrict__ row) const
   {
      row[0] = (double)n; row[1] = (double)bad; row[2] = sumQ4; row[3] = sumQ6; row[4] = sumW4; row[5] = sumW6;
      row[6] = minQ6; row[7] = (double)gid; row[8] = maxQ6; row[9] = (double)above;
   }
   __device__ static SteinhardtSum fromRow(const double* __restrict__ row)
   {
      return SteinhardtSum{ row[2], row[3], row[4], row[5], row[6], row[8], (int)row[7], (int)row[0], (int)row[1], (int)row[9] };
   }
};

// stage 1: the four planes of the occupied slots; an invalid atom counts and stays out of the rest
__global__ __launch_bounds__(256)
void Steinhardt_Summary(const real_t* __restrict__ planes, size_t plane, const int* __restrict__ nAtoms, const int* __restrict__ gid, int cap,
                        double threshold, double* __restrict__ partial)
{
   summaryOfSlots<SteinhardtSum>(plane, nAtoms, cap, partial, [&](size_t o) {
      const double q4 = (double)planes[o], q6 = (double)planes[plane + o], w4 = (double)planes[2 * plane + o], w6 = (double)planes[3 * plane + o];
      SteinhardtSum c = SteinhardtSum::empty();
      if (q4 != q4) c.bad = 1;
      else { c.sumQ4 = q4; c.sumQ6 = q6; c.sumW4 = w4; c.sumW6 = w6; c.minQ6 = q6; c.maxQ6 = q6; c.gid = gid[o]; c.n = 1; c.above = q6 >= threshold ? 1 : 0; }
      return c;
   });
}

// stage 2: the rows -> out[STEINHARDT_SUM_N]
__global__ __launch_bounds__(256)
void Steinhardt_SummaryFinal(const double* __restrict__ partial, int nPartial, double* __restrict__ out)
{
   summaryOfRows<SteinhardtSum>(partial, nPartial, out);
}
