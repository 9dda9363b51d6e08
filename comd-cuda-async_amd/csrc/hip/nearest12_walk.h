// nearest12_walk.h -- the "12 nearest neighbours of a lane's atom" walk and merge that CentroSym_thread_atom (csp_kernels.h, which describes it) and
// Cna_thread_atom (cna_kernels.h) share.  NOT a header of declarations: it is the text of the walk, included inside the kernel's loop over its units of
// work, so that both kernels compile the very statements the csp kernel had in its own body.  (As a __forceinline__ function taking the sets by reference
// the same statements cost CentroSym_thread_atom its allocation in the double build: 128 VGPRs and 104 to 1624 bytes of scratch instead of 124 and 0.)
//
// In scope at the point of inclusion:
//   v                  the kernel's argument record with rx, ry, rz, nAtoms, nbr, cap, chunks, rc2 (and rCoord2 when NN12_COORD keeps its argument)
//   w, lane            the unit of work, cell * v.chunks + chunk, and the lane
//   NN12_COORD(x)      a macro: x for a kernel that counts the coordination number, nothing otherwise
// It `continue`s on an empty chunk.  After it: me = the lane's slot, xi, yi, zi its position, d[] / id[] = r^2 and slot of the 12 nearest in ascending
// order (id[11] < 0: fewer than 12 inside the cutoff), coord (with NN12_COORD), and active && q == 0 = the lane holds an atom and is the copy of a
// replicated chunk that writes the result.
      const int iBox = uniform((int)(w / v.chunks));
      const int first = uniform((int)(w - (long)iBox * v.chunks)) * WAVE;
      const int ni = uniform(v.nAtoms[iBox]);
      if (first >= ni) continue;
      // a chunk of m <= 32 atoms is replicated: reps copies of its atoms, copy q walks the stencil cells q, q + reps, ... (as PairHist_thread_atom)
      const int m = ni - first < WAVE ? ni - first : WAVE;
      int reps = 1;
      while (reps < 16 && 2 * reps * m <= WAVE) reps *= 2;
      const int span = WAVE / reps, q = lane / span;
      const int ia = first + (lane & (span - 1));
      const bool active = ia < first + m;
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
      const int* __restrict__ nb = v.nbr + (size_t)iBox * 27;
      if (reps > 1) {
         for (int k = q; k < 27; k += reps) {
            const int jBox = nb[k];
            const int nj = v.nAtoms[jBox];
            const int base = jBox * v.cap;
            for (int j = 0; j < nj; ++j) test(v.rx[base + j], v.ry[base + j], v.rz[base + j], base + j);
         }
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
      } else for (int k = 0; k < 27; ++k) {
         const int jBox = uniform(nb[k]);
         const int nj = uniform(v.nAtoms[jBox]);
         const int base = jBox * v.cap;
         const real_t* __restrict__ qx = v.rx + base;
         const real_t* __restrict__ qy = v.ry + base;
         const real_t* __restrict__ qz = v.rz + base;
         int j = 0;
         for (; j + 8 <= nj; j += 8) {
            real_t xs[8], ys[8], zs[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { xs[u] = qx[j + u]; ys[u] = qy[j + u]; zs[u] = qz[j + u]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) test(xs[u], ys[u], zs[u], base + j + u);
         }
         for (; j < nj; ++j) test(qx[j], qy[j], qz[j], base + j);
      }
