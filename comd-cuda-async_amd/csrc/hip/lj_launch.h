// lj_launch.h -- the LJ launch layer: the kernel arguments, the margins of the pruning tests, the grid and candidate lists of thread_atom, and which kernel a force call
// runs on.  Host code, part of comd_device.hip's translation unit (it uses HIP_CHECK, LAUNCH_CHECK, S, ForceTimer, dalloc, allowDynamicLds, ceilDiv, tuningOf and legsOf of
// that file).  The analytic pair and the -I table share every launch shape: one dispatch each, the table kernels take the TableView as one more argument.
#pragma once

static NlView nlView(SimGpu* sim)
{
   NeighborListGpu* n = &sim->atoms.neighborList;
   if (!n->list && !n->list16) { fprintf(stderr, "the *_nl methods need Verlet lists: allocate with GpuConfig.skinDistance > 0\n"); exit(-1); }
   if (n->nBuilds == 0) { fprintf(stderr, "the *_nl methods need buildNeighborListGpu before the first force call\n"); exit(-1); }
   NlView v; v.list = n->list; v.count = n->nNeighbors; v.maxNbr = n->maxNeighbors;
   return v;
}

static LjArgs makeLjArgs(SimGpu* sim, int num_cells, int* cells_list)
{
   LjArgs a;
   a.rx = sim->atoms.r.x; a.ry = sim->atoms.r.y; a.rz = sim->atoms.r.z;
   a.fx = sim->atoms.f.x; a.fy = sim->atoms.f.y; a.fz = sim->atoms.f.z; a.e = sim->atoms.e;
   a.nAtoms = sim->boxes.nAtoms; a.nbr = sim->neighbor_cells; a.cells = cells_list;
   a.nCells = num_cells; a.cap = sim->maxAtoms;
   const double sigma = sim->lj_pot.sigma, rc = sim->lj_pot.cutoff;
   a.rc2 = rc * rc;
   a.s6 = sigma * sigma * sigma * sigma * sigma * sigma;
   a.s6x2 = 2.0 * (sigma * sigma * sigma * sigma * sigma * sigma);
   const double rc6 = a.s6 / (a.rc2 * a.rc2 * a.rc2);
   a.eShift = rc6 * (rc6 - 1.0);                 // POT_SHIFT 1.0
   a.eps = sim->lj_pot.epsilon;
   return a;
}

// Margins of the point-to-box pruning test (LJ_WaveCandidates, LJ_Force_cta_cell_boxes): the test may keep a candidate it need not, never drop one a
// lane would accept.  A relative margin on rc^2 and on the half widths covers the arithmetic of the distance; the box CENTRE is formed from absolute
// coordinates, whose ulp grows with the box (float: 3e-5 A at 289 A, 1.2e-4 A beyond 1024 A -- ADVICE r2), so the cutoff is also pushed out by eight
// ulps of the largest coordinate this rank can see (local domain + one halo cell), per axis.
static void ljBoxMargins(const SimGpu* sim, real_t rc2, real_t* rc2Box, real_t* grow)
{
   const double rel = sizeof(real_t) == 8 ? 1e-12 : 1e-5, eps = sizeof(real_t) == 8 ? 2.220446049250313e-16 : 1.1920929e-07;
   double big = 0.0;
   for (int a = 0; a < 3; ++a) {
      const double cellW = 1.0 / sim->boxes.invBoxSize[a];
      const double lo = fabs((double)sim->boxes.localMin[a] - cellW), hi = fabs((double)sim->boxes.localMax[a] + cellW);
      if (lo > big) big = lo;
      if (hi > big) big = hi;
   }
   const double rc = sqrt((double)rc2) * (1.0 + rel) + 8.0 * 1.7320508 * eps * big;
   *rc2Box = (real_t)(rc * rc);
   *grow = (real_t)(1.0 + rel);
}

// The list build of thread_atom (LJ_WaveCandidates) makes the same test in SINGLE precision on positions relative to the corner of the local domain
// (LJ_PackPositions): the conversion moves a coordinate by half an ulp of the largest relative coordinate (local domain + one halo cell on either side),
// the arithmetic of the box distance is good to ~1e-6 relative -- the cutoff is pushed out by 1e-5 relative + eight such ulps per axis.
static void ljBoxMarginsF(const SimGpu* sim, real_t rc2, float* rc2Box, float* grow)
{
   const double rel = 1e-5, eps = 1.1920929e-07;
   double big = 0.0;
   for (int a = 0; a < 3; ++a) {
      const double ext = (double)sim->boxes.localMax[a] - (double)sim->boxes.localMin[a] + 2.0 / sim->boxes.invBoxSize[a];
      if (ext > big) big = ext;
   }
   const double rc = sqrt((double)rc2) * (1.0 + rel) + 8.0 * 1.7320508 * eps * big;
   *rc2Box = (float)(rc * rc * (1.0 + 2.0 * eps));
   *grow = (float)(1.0 + rel);
}

// The grid and the candidate lists of a thread_atom force call, shared by the analytic and the table kernel
struct LjThreadAtomLaunch { int w, wavesPerBlock; unsigned nBlocks; bool prune; LjWaveLists wl; };

// thread_atom (the BASELINE-named kernel): candidate lists (launched here), and the grid the force kernel needs
static LjThreadAtomLaunch prepareLjThreadAtom(SimGpu* sim, const LjArgs& a, int num_cells, int* cells_list, comdStream_t stream)
{
   // Measured on MI355X (LJ 80^3): a workgroup of the 3 live waves per cell runs the kernel in 3.94 ms, cap/64 = 4 waves per cell (the
   // tail wave exits at once) in 4.72 ms, single-wave workgroups in 5.64 ms.
   // waves per cell: sized to the occupancy the host last saw (+16 atoms of slack), never more than cap/64.  Cells that outgrow the
   // estimate stay correct (their waves take extra chunks).  COMD_LJ_WAVES=k forces k (tests use 1 to exercise the extra-chunk path).
   int w = sim->maxAtoms / 64;
   if (sim->max_atoms_cell > 0 && (sim->max_atoms_cell + 16 + 63) / 64 < w) w = (sim->max_atoms_cell + 16 + 63) / 64;
   const ComdTuning& tune = tuningOf(sim);
   if (tune.ljWaves && tune.ljWaves < w) w = tune.ljWaves;
   const int wavesPerBlock = w <= 4 ? w : 4;
   const unsigned nBlocks = w <= 4 ? (unsigned)num_cells : (unsigned)ceilDiv((long)num_cells * w, 4);
   // candidate lists of the waves (lj_kernels.h): rows sized for 70 % of the fullest stencil the host has seen -- the part of 27 cells
   // within the cutoff of a whole cell's box is 76 %, of a 64-atom slab of it 61 % -- and a wave whose row is too short walks the stencil.
   // COMD_LJ_PRUNE=0 switches the lists off (A/B measurements); COMD_LJ_LIST_CAP=n forces rows of n entries (tests: the fallback).
   const bool pruneEnv = tune.ljPrune;
   LjPotentialGpu* lj = &sim->lj_pot;
   if (pruneEnv && !lj->waveCand && lj->packedCap == 0) {
      // the fullest cell right now (one blocking read, once per simulation; SimGpu.max_atoms_cell may not have been filled in yet)
      std::vector<int> counts((size_t)sim->boxes.nTotalBoxes);
      HIP_CHECK(hipMemcpyAsync(counts.data(), sim->boxes.nAtoms, counts.size() * sizeof(int), hipMemcpyDeviceToHost, S(stream)));
      HIP_CHECK(hipStreamSynchronize(S(stream)));
      int fullest = sim->max_atoms_cell;
      for (int c : counts) if (c > fullest) fullest = c;
      const int occ = fullest + 16 < sim->maxAtoms ? fullest + 16 : sim->maxAtoms;
      lj->waveCandWaves = w;
      lj->waveCandCap = ((int)(0.70 * 27 * occ) + 7) & ~7;
      if (tune.ljListCap) lj->waveCandCap = tune.ljListCap;
      lj->packedCap = ((occ + 7) & ~7) < sim->maxAtoms ? ((occ + 7) & ~7) : sim->maxAtoms;     // a stencil with a fuller cell falls back to the walk
      // list entries are 32-bit byte offsets into the packed records
      // ~250 B of list per atom (18 GB at 256^3) + the packed records (2.9 GB each): when that does not fit what the device has free (keeping 2 GB
      // for everything allocated later), or the 32-bit offsets cannot reach the records, this simulation walks the stencil as round 1 did
      const double listBytes = (double)sim->boxes.nLocalBoxes * lj->waveCandWaves * lj->waveCandCap * 4.0 + (double)sim->boxes.nLocalBoxes * lj->waveCandWaves * 8.0
                               + (sim->interior_stream ? 2.0 : 1.0) * (double)sim->boxes.nTotalBoxes * lj->packedCap * (sizeof(LjPos4) + sizeof(float4));
      size_t freeB = 0, totalB = 0;
      HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
      if ((double)sim->boxes.nTotalBoxes * lj->packedCap * sizeof(LjPos4) >= 4294967296.0) lj->packedCap = -1;     // no lists for this simulation
      else if (listBytes + 2.0e9 > (double)freeB || listBytes > 1.0e6 * tune.ljListBudgetMb) {
         fprintf(stderr, "Rank %d: LJ candidate lists need %.1f GB, %.1f GB are free: running without them (the plain 27-cell walk, ~1.4x slower)\n",
                 g_rank, listBytes / 1e9, (double)freeB / 1e9);
         lj->packedCap = -1;
      } else {
         // Everything the lists need is allocated HERE, and a refusal is not fatal: ranks that share a device can all see the memory free and then not all
         // get it -- whoever is refused runs the plain walk, and says so (bench.py records force_path.lj_candidate_lists_active).
         auto tryAlloc = [](size_t bytes) { void* p = nullptr; if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) { (void)hipGetLastError(); p = nullptr; } return p; };
         const size_t recs = (size_t)sim->boxes.nTotalBoxes * lj->packedCap * 4;
         lj->waveCand = (unsigned*)tryAlloc((size_t)sim->boxes.nLocalBoxes * lj->waveCandWaves * lj->waveCandCap * sizeof(unsigned));
         lj->waveCandCount = (int*)tryAlloc((size_t)sim->boxes.nLocalBoxes * lj->waveCandWaves * 2 * sizeof(int));
         bool ok = lj->waveCand && lj->waveCandCount;
         for (int k = 0; k < (sim->interior_stream ? 2 : 1) && ok; ++k) {
            lj->packedR[k] = (real_t*)tryAlloc(recs * sizeof(real_t));
            lj->packedF[k] = (float*)tryAlloc(recs * sizeof(float));
            ok = lj->packedR[k] && lj->packedF[k];
         }
         if (!ok) {
            void* ps[6] = { lj->waveCand, lj->waveCandCount, lj->packedR[0], lj->packedF[0], lj->packedR[1], lj->packedF[1] };
            for (void* q : ps) if (q) (void)hipFree(q);
            lj->waveCand = nullptr; lj->waveCandCount = nullptr; lj->packedR[0] = lj->packedR[1] = nullptr; lj->packedF[0] = lj->packedF[1] = nullptr;
            fprintf(stderr, "Rank %d: the device refused the %.1f GB of the LJ candidate lists: running without them (the plain 27-cell walk, ~1.4x slower)\n", g_rank, listBytes / 1e9);
            lj->packedCap = -1;
         }
      }
   }
   const bool prune = pruneEnv && lj->waveCand;
   LjWaveLists wl; memset(&wl, 0, sizeof wl);
   if (prune) {
      // the force may be split over two streams (-a 1: interior cells while the halo exchange is in flight, boundary cells after it):
      // each stream packs the positions it is about to read into its own array
      const int which = (cells_list && stream != sim->interior_stream) ? 1 : 0;
      if (!lj->packedR[which]) {
         lj->packedR[which] = dalloc<real_t>((size_t)sim->boxes.nTotalBoxes * lj->packedCap * 4, false);
         lj->packedF[which] = dalloc<float>((size_t)sim->boxes.nTotalBoxes * lj->packedCap * 4, false);
      }
      wl.cand = lj->waveCand; wl.pos = (const LjPos4*)lj->packedR[which]; wl.posF = (const float4*)lj->packedF[which]; wl.count = (int2*)lj->waveCandCount;
      wl.candCap = lj->waveCandCap; wl.wavesMax = lj->waveCandWaves; wl.capP = lj->packedCap;
      ljBoxMarginsF(sim, a.rc2, &wl.rc2BoxF, &wl.growF);
      // interior cells never have a halo cell in their stencil, and the halo cells are being filled while they run
      const int packCells = (cells_list && stream == sim->interior_stream) ? sim->boxes.nLocalBoxes : sim->boxes.nTotalBoxes;
      ForceTimer aux(sim, S(stream), 1);               // the list build of this evaluation (bench.py: force_evaluation_ms = kernel + this)
      hipLaunchKernelGGL(LJ_PackPositions, dim3((unsigned)ceilDiv((long)packCells * lj->packedCap, 256)), dim3(256), 0, S(stream),
                         a.rx, a.ry, a.rz, a.nAtoms, (LjPos4*)lj->packedR[which], (float4*)lj->packedF[which], a.cap, lj->packedCap, packCells, a.rc2,
                         sim->boxes.localMin[0], sim->boxes.localMin[1], sim->boxes.localMin[2]);
      hipLaunchKernelGGL(LJ_WaveCandidates, dim3((unsigned)ceilDiv(num_cells, 4)), dim3(256), 0, S(stream), a, wl, w);
   }
   LjThreadAtomLaunch L; L.w = w; L.wavesPerBlock = wavesPerBlock; L.nBlocks = nBlocks; L.prune = prune; L.wl = wl;
   return L;
}

static TableView ljTableView(const SimGpu* sim)
{
   const InterpolationObjectGpu& t = sim->lj_pot.lj_interpolation;
   TableView tv; tv.v = t.values; tv.x0 = t.x0; tv.xn = t.xn; tv.invDx = t.invDx; tv.invDxHalf = t.invDxHalf; tv.invDxXx0 = t.invDxXx0;
   return tv;
}

// One launch shape, two pair functions: the analytic kernel or, with -I, its table form (lj_table_kernels.h), which takes the same arguments and the TableView behind them.
template <class KA, class KT, class... A>
static void launchLjPair(SimGpu* sim, bool table, KA analytic, KT tabled, dim3 grid, dim3 block, size_t lds, comdStream_t stream, const A&... args)
{
   if (lds) allowDynamicLds(table ? (const void*)tabled : (const void*)analytic, lds);
   if (table) hipLaunchKernelGGL(tabled, grid, block, lds, S(stream), args..., ljTableView(sim));
   else       hipLaunchKernelGGL(analytic, grid, block, lds, S(stream), args...);
}

// fn(std::true_type()) when the coming energy read needs e[] (comdSetEnergyNeeded), fn(std::false_type()) when not: the ENERGY parameter of the force kernels
template <class F>
static void withEnergy(const SimGpu* sim, F fn) { if (sim->needEnergy) fn(std::true_type()); else fn(std::false_type()); }

// table: the -I kernel on the same grid and lists
static void launchLjThreadAtom(SimGpu* sim, const LjArgs& a, int num_cells, int* cells_list, comdStream_t stream, bool table)
{
   const LjThreadAtomLaunch L = prepareLjThreadAtom(sim, a, num_cells, cells_list, stream);
   const bool prune = L.prune;
   const bool prefetch = prune && !table && tuningOf(sim).ljPrefetch;      // (the -I kernel is instantiated without the prefetch)
   { ForceLegs& legs = legsOf(sim); legs.ljWaves = L.w; legs.ljLists = prune; legs.ljListCap = prune ? L.wl.candCap : 0; legs.ljPrefetch = prefetch; }
   ForceTimer timer(sim, S(stream));                     // the force kernel proper (bench.py's roofline line; rocprof must agree with it)
   withEnergy(sim, [&](auto energy) {
      constexpr bool E = decltype(energy)::value;
      const dim3 grid(L.nBlocks), block(64 * L.wavesPerBlock);
      if (prefetch)   launchLjPair(sim, table, LJ_Force_thread_atom<E, true>,  LJ_Force_thread_atom_table<E, true>,  grid, block, 0, stream, a, L.w, L.wl);
      else if (prune) launchLjPair(sim, table, LJ_Force_thread_atom_plain<E>,  LJ_Force_thread_atom_table<E, true>,  grid, block, 0, stream, a, L.w, L.wl);
      else            launchLjPair(sim, table, LJ_Force_thread_atom<E, false>, LJ_Force_thread_atom_table<E, false>, grid, block, 0, stream, a, L.w, L.wl);
   });
   LAUNCH_CHECK();
}

// table: -I (lj_pot.lj_interpolation), thread_atom and both list formats of thread_atom_nl
static void ljForce(SimGpu* sim, int num_cells, int* cells_list, int method, comdStream_t stream, bool table)
{
   if (num_cells <= 0) return;
   LjArgs a = makeLjArgs(sim, num_cells, cells_list);
   if (table) {
      if (!sim->lj_pot.lj_interpolation.values) { fprintf(stderr, "ljForceGpu: interpolation requested but there is no LJ table: call initLJinterpolation first\n"); exit(-1); }
      if (method == CTA_CELL) { fprintf(stderr, "ljForceGpu: interpolated LJ (-I) runs with thread_atom and thread_atom_nl, not cta_cell\n"); exit(-1); }
   }
   if (method != THREAD_ATOM_NL && method != WARP_ATOM_NL && method != CTA_CELL) { launchLjThreadAtom(sim, a, num_cells, cells_list, stream, table); return; }
   ForceTimer timer(sim, S(stream));
   if ((method == THREAD_ATOM_NL || method == WARP_ATOM_NL) && sim->atoms.neighborList.slabFormat) {
      NeighborListGpu* n = &sim->atoms.neighborList;
      (void)nlView(sim);
      NlSlabView v; v.list = n->list16; v.count = n->nNeighbors; v.rows = n->slabRows;
      const int threads = ((n->maxCellAtoms + 63) / 64) * 64;
      const size_t lds = (size_t)3 * n->maxSlabAtoms * sizeof(real_t);
      withEnergy(sim, [&](auto energy) {
         constexpr bool E = decltype(energy)::value;
         launchLjPair(sim, table, LJ_Force_nl_slabs<E>, LJ_Force_nl_slabs_table<E>, dim3(num_cells), dim3(threads), lds, stream, a, v, n->maxSlabAtoms);
      });
   } else if (method == THREAD_ATOM_NL || method == WARP_ATOM_NL) {
      const NlView nl = nlView(sim);
      const unsigned nBlocks = (unsigned)ceilDiv((long)num_cells * sim->maxAtoms, 256);
      withEnergy(sim, [&](auto energy) {
         constexpr bool E = decltype(energy)::value;
         launchLjPair(sim, table, LJ_Force_thread_atom_nl<E>, LJ_Force_thread_atom_nl_table<E>, dim3(nBlocks), dim3(256), 0, stream, a, nl);
      });
   } else if (method == CTA_CELL) {
      const size_t lds = ljCtaLdsBytes(sim->maxAtoms);
      allowDynamicLds((const void*)LJ_Force_cta_cell<0, true>, lds); allowDynamicLds((const void*)LJ_Force_cta_cell<0, false>, lds);
      allowDynamicLds((const void*)LJ_Force_cta_cell<1, true>, lds); allowDynamicLds((const void*)LJ_Force_cta_cell<1, false>, lds);
      allowDynamicLds((const void*)LJ_Force_cta_cell<2, true>, lds); allowDynamicLds((const void*)LJ_Force_cta_cell<2, false>, lds);
      // threads = atoms of the fullest cell the host has seen (+16), rounded to whole waves, at most 256; each thread can own two atoms
      int threads = sim->maxAtoms < 256 ? sim->maxAtoms : 256;
      // (not with pairlists: their bits are per wave, so the thread -> atom map must not change between the generating call and the users)
      if (sim->atoms.neighborList.slabFormat != 3 && sim->max_atoms_cell > 0 && ((sim->max_atoms_cell + 16 + 63) / 64) * 64 < threads)
         threads = ((sim->max_atoms_cell + 16 + 63) / 64) * 64;
      if (sim->maxAtoms > 2 * threads) { fprintf(stderr, "ljForceGpu: cta_cell supports at most 512 atoms per cell\n"); exit(-1); }
      NeighborListGpu* n = &sim->atoms.neighborList;
      LjPairlist pl; pl.words = n->pairlist; pl.wavesMax = n->pairlistWaves;
      pl.plCut2 = (sim->lj_pot.cutoff + n->skinDistance) * (sim->lj_pot.cutoff + n->skinDistance);
#define LAUNCH_CTA(PLV) do { if (sim->needEnergy) hipLaunchKernelGGL((LJ_Force_cta_cell<PLV, true>), dim3(num_cells), dim3(threads), lds, S(stream), a, sim->status, pl); \
                            else              hipLaunchKernelGGL((LJ_Force_cta_cell<PLV, false>), dim3(num_cells), dim3(threads), lds, S(stream), a, sim->status, pl); } while (0)
      legsOf(sim).ljCtaForm = n->slabFormat == 3 ? 3 : tuningOf(sim).ljCtaSlabs ? 2 : 1;
      if (n->slabFormat != 3 && !tuningOf(sim).ljCtaSlabs) {
         // the default form: every wave stages its own box-pruned candidates (COMD_LJ_CTA_SLABS=1: the slab kernel, for A/B runs)
         real_t rc2Box, grow;
         ljBoxMargins(sim, a.rc2, &rc2Box, &grow);
         const size_t ldsB = ljCtaBoxesLdsBytes(threads);
         if (sim->needEnergy) hipLaunchKernelGGL(LJ_Force_cta_cell_boxes<true>, dim3(num_cells), dim3(threads), ldsB, S(stream), a, rc2Box, grow);
         else                 hipLaunchKernelGGL(LJ_Force_cta_cell_boxes<false>, dim3(num_cells), dim3(threads), ldsB, S(stream), a, rc2Box, grow);
      }
      else if (n->slabFormat != 3)               LAUNCH_CTA(0);
      else if (n->nBuilds == 0) { fprintf(stderr, "ljForceGpu: -L needs buildNeighborListGpu before the first force call\n"); exit(-1); }
      else if (n->pairlistBuildId != n->nBuilds) LAUNCH_CTA(1);
      else                                       LAUNCH_CTA(2);
#undef LAUNCH_CTA
   }
   LAUNCH_CHECK();
}

extern "C" void ljForceGpuAsync(SimGpu* sim, int num_cells, int* cells_list, int method, comdStream_t stream)
{
   ljForce(sim, num_cells, cells_list, method, stream, sim->lj_pot.lj_interpolation.values != nullptr);
}

extern "C" void ljForceGpu(SimGpu* sim, int interpolation, int num_cells, int* cells_list, real_t plcutoff, int method)
{
   (void)plcutoff;
   ljForce(sim, num_cells, cells_list, method, nullptr, interpolation != 0);
}
