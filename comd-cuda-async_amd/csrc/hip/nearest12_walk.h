// nearest12_walk.h -- the "12 nearest neighbours of a lane's atom" selection and merge that CentroSym_thread_atom (csp_kernels.h, which describes it) and
// Cna_thread_atom (cna_kernels.h) share, on the chunk walk of stencil_walk.h.  NOT a header of declarations: it is text, included inside the body the
// kernel hands to forEachChunk, so that both kernels compile the very statements the csp kernel had in its own body.  (As a __forceinline__ function
// taking the sets by reference, or handing them to a stage lambda, the same statements cost CentroSym_thread_atom its allocation in the double build:
// 128 VGPRs and 20 to 1624 bytes of scratch instead of 124 and 0.)
//
// In scope at the point of inclusion:
//   v                  the kernel's argument record: StencilArgs with rc2 (and rCoord2 when NN12_COORD keeps its argument)
//   iBox, first, reps, span, q, ia, active, lane        the values forEachChunk hands to the body, and the lane
//   NN12_COORD(x)      a macro: x for a kernel that counts the coordination number, nothing otherwise
// After it: me = the lane's slot, xi, yi, zi its position, d[] / id[] = r^2 and slot of the 12 nearest in ascending order (id[11] < 0: fewer than 12
// inside the cutoff), coord (with NN12_COORD), and active && q == 0 = the lane holds an atom and is the copy of a replicated chunk that writes the result.
      const int me = iBox * v.cap + (active ? ia : first);
      const real_t xi = v.rx[me], yi = v.ry[me], zi = v.rz[me];

      // The four sets are arrays inside structs.  A bare array that is still in memory when the compiler's promote-alloca pass runs (before the loops are
      // unrolled) may be made one 12-wide vector, as far as that pass's register budget reaches.  In CentroSym_thread_atom none of the four was (its IR holds no
      // vector); in Cna_thread_atom, and in a kernel of the walk alone, pd[] was, and the 24-register tuples cost 1 to 1.6 kB of scratch in the double build
      // (12 bytes with the pass switched off).  The pass leaves structs alone.
      struct { real_t v[CSP_NN]; } dSet; struct { int v[CSP_NN]; } idSet;
      real_t (&d)[CSP_NN] = dSet.v; int (&id)[CSP_NN] = idSet.v;
#pragma unroll
      for (int k = 0; k < CSP_NN; ++k) { d[k] = active ? v.rc2 : R(0.0); id[k] = -1; }      // an idle lane takes nothing
      NN12_COORD(int coord = 0;)
      auto test = [&](real_t xj, real_t yj, real_t zj, int slot) {
         const real_t dx = xj - xi, dy = yj - yi, dz = zj - zi;
         const real_t r2 = dx*dx + dy*dy + dz*dz;
         const bool other = slot != me;
         NN12_COORD(coord += (other && r2 < v.rCoord2) ? 1 : 0;)
         if (other && r2 < d[CSP_NN - 1]) cspOffer<CSP_NN>(d, id, r2, slot);
      };
      stencilWalk<int>(v, iBox, reps, q, test);
      if (reps > 1) {
         // the copies' sets into one: after the doubling over s every lane holds the 12 nearest of the copies lane ^ s, lane ^ 2s, ... as well
         for (int s = span; s < WAVE; s <<= 1) {
            const int addr = (lane ^ s) << 2;
            struct { real_t v[CSP_NN]; } pdSet; struct { int v[CSP_NN]; } piSet;
            real_t (&pd)[CSP_NN] = pdSet.v; int (&pi)[CSP_NN] = piSet.v;
#pragma unroll
            for (int k = 0; k < CSP_NN; ++k) { pd[k] = bpermuteAddrR(d[k], addr); pi[k] = __builtin_amdgcn_ds_bpermute(addr, id[k]); }
            NN12_COORD(coord += __builtin_amdgcn_ds_bpermute(addr, coord);)
            // the lower copy's entries win ties in both lanes of a pair: the upper copy's set is rebuilt from the lower one's
            const bool upper = (lane & s) != 0;
#pragma unroll
            for (int k = 0; k < CSP_NN; ++k) {
               const real_t td = d[k]; const int ti = id[k];
               d[k] = upper ? pd[k] : td; id[k] = upper ? pi[k] : ti;
               pd[k] = upper ? td : pd[k]; pi[k] = upper ? ti : pi[k];
            }
#pragma unroll
            for (int k = 0; k < CSP_NN; ++k)
               if (pi[k] >= 0 && pd[k] < d[CSP_NN - 1]) cspOffer<CSP_NN>(d, id, pd[k], pi[k]);
         }
      }
