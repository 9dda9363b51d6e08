// analysis_launch.h -- the launch layer of the analyses, computeVirial ... computeStructureFactor (comd_hip.h): none of them is in the reference.  Host code,
// part of comd_device.hip's translation unit (it uses HIP_CHECK, LAUNCH_CHECK, S, dalloc, allowDynamicLds, ceilDiv, of that file, makeLjArgs and ljTableView of lj_launch.h).
#pragma once

// The entry points of the chunk walk (stencil_walk.h) share their prologue and the fields of the walk.
// They run on the boundary stream; -a 1: the interior cells' force work is done first
static hipStream_t analysisStream(SimGpu* sim)
{
   if (sim->interior_stream) HIP_CHECK(hipStreamSynchronize(S(sim->interior_stream)));
   return S(sim->boundary_stream);
}

static void fillStencilArgs(StencilArgs& v, const SimGpu* sim)
{
   v.rx = sim->atoms.r.x; v.ry = sim->atoms.r.y; v.rz = sim->atoms.r.z;
   v.nAtoms = sim->boxes.nAtoms; v.nbr = sim->neighbor_cells;
   v.nLocalBoxes = sim->boxes.nLocalBoxes; v.cap = sim->maxAtoms; v.chunks = ceilDiv(sim->maxAtoms, WAVE);
}

// the slots of the local cells: the length of a by-slot plane
static size_t localSlots(const SimGpu* sim) { return (size_t)sim->boxes.nLocalBoxes * sim->maxAtoms; }

// the cutoff of the potential: the largest radius the 27-cell walk is good for
static real_t pairCutoff(const SimGpu* sim) { return sim->do_eam ? sim->eam_pot.cutoff : sim->lj_pot.cutoff; }

// the kernels of nearest12_walk.h compute slots in int
static void refuseSlotsBeyondInt(const SimGpu* sim, const char* who)
{
   if ((double)sim->boxes.nTotalBoxes * sim->maxAtoms >= 2147483648.0) { fprintf(stderr, "%s: more than 2^31 slots\n", who); exit(-1); }
}

// fn(pair, rc2) with the pair function of the simulation's force path (virial_kernels.h) and its squared cutoff: one kernel instance per functor type
template <class FN>
static void withPairFunction(SimGpu* sim, FN fn)
{
   if (!sim->do_eam) {
      const LjArgs a = makeLjArgs(sim, sim->boxes.nLocalBoxes, nullptr);
      if (sim->lj_pot.lj_interpolation.values) { VirialLjTable p; p.t = ljTableView(sim); fn(p, a.rc2); }
      else { VirialLj p; p.a = a; fn(p, a.rc2); }
   } else {
      const EamPotentialGpu& e = sim->eam_pot;
      auto eam = [&](auto p) { p.phi = e.phi; p.rho = e.rho; p.phiS = e.phiS; p.rhoS = e.rhoS; p.dfEmbed = e.dfEmbed; p.dfi = R(0.0); fn(p, (real_t)(e.cutoff * e.cutoff)); };
      if (e.phiS.coefficients && e.rhoS.coefficients) eam(VirialEam<true>()); else eam(VirialEam<false>());
   }
}

// Not in the reference: the pair virial and the kinetic tensor (virial_kernels.h), one kernel instance per pair function of the force paths
extern "C" void computeVirial(SimGpu* sim, real_t* out12)
{
   hipStream_t st = analysisStream(sim);
   if (!sim->virialBuf) sim->virialBuf = dalloc<double>((size_t)(VIRIAL_BLOCKS + 1) * VIRIAL_N, false);
   VirialArgs v;
   fillStencilArgs(v, sim);
   v.px = sim->atoms.p.x; v.py = sim->atoms.p.y; v.pz = sim->atoms.p.z;
   v.iSpecies = sim->atoms.iSpecies; v.speciesMass = sim->species_mass;
   v.partial = sim->virialBuf;
   double* out = sim->virialBuf + (size_t)VIRIAL_BLOCKS * VIRIAL_N;
   withPairFunction(sim, [&](auto p, real_t rc2) {
      v.rc2 = rc2;
      hipLaunchKernelGGL(Virial_thread_atom<decltype(p)>, dim3(VIRIAL_BLOCKS), dim3(256), 0, st, v, p);
   });
   hipLaunchKernelGGL(Virial_Final, dim3(1), dim3(256), 0, st, sim->virialBuf, VIRIAL_BLOCKS, out);
   LAUNCH_CHECK();
   double h[VIRIAL_N];
   HIP_CHECK(hipMemcpyAsync(h, out, sizeof h, hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
   for (int c = 0; c < VIRIAL_N; ++c) out12[c] = (real_t)h[c];
}

// Not in the reference: the work list of the face kernel of computeVirialFdotr (fdotr_kernels.h).  Every id is checked here: the kernel trusts the rows
extern "C" void comdSetFacePairsGpu(SimGpu* sim, const int* rows5, int nRows)
{
   for (int k = 0; k < nRows; ++k) {
      const int* r = rows5 + 5 * (size_t)k;
      const bool ok = r[0] >= 0 && r[0] < sim->boxes.nLocalBoxes && r[1] >= sim->boxes.nLocalBoxes && r[1] < sim->boxes.nTotalBoxes
                      && r[2] >= -1 && r[2] <= 1 && r[3] >= -1 && r[3] <= 1 && r[4] >= -1 && r[4] <= 1;
      if (!ok) { fprintf(stderr, "comdSetFacePairsGpu: row %d (%d, %d, %d, %d, %d) is out of range\n", k, r[0], r[1], r[2], r[3], r[4]); exit(-1); }
   }
   if (sim->fdotrRows) { HIP_CHECK(hipStreamSynchronize(S(sim->boundary_stream))); HIP_CHECK(hipFree(sim->fdotrRows)); }
   sim->fdotrRows = dalloc<int>(5 * (size_t)(nRows > 0 ? nRows : 1), false);
   if (nRows > 0) HIP_CHECK(hipMemcpy(sim->fdotrRows, rows5, 5 * (size_t)nRows * sizeof(int), hipMemcpyHostToDevice));
   sim->fdotrNRows = nRows;
}

// Not in the reference: the pair virial from the forces on the device and the periodic face pairs (fdotr_kernels.h), one face-kernel instance per pair function
extern "C" void computeVirialFdotr(SimGpu* sim, const double box[3], real_t* out12)
{
   hipStream_t st = analysisStream(sim);
   if (!sim->fdotrRows) { fprintf(stderr, "computeVirialFdotr: no work list (comdSetFacePairsGpu)\n"); exit(-1); }
   const dim3 atomsGrid = integratorGrid(sim);
   const int nPartial = (int)atomsGrid.x + FDOTR_FACE_BLOCKS;
   if (!sim->fdotrBuf) sim->fdotrBuf = dalloc<double>((size_t)(nPartial + 1) * VIRIAL_N, false);
   double* out = sim->fdotrBuf + (size_t)nPartial * VIRIAL_N;
   FdotrAtomsArgs a;
   a.rx = sim->atoms.r.x; a.ry = sim->atoms.r.y; a.rz = sim->atoms.r.z;
   a.fx = sim->atoms.f.x; a.fy = sim->atoms.f.y; a.fz = sim->atoms.f.z;
   a.px = sim->atoms.p.x; a.py = sim->atoms.p.y; a.pz = sim->atoms.p.z;
   a.iSpecies = sim->atoms.iSpecies; a.speciesMass = sim->species_mass; a.nAtoms = sim->boxes.nAtoms;
   a.nLocalBoxes = sim->boxes.nLocalBoxes; a.cap = sim->maxAtoms; a.laneBits = integratorLaneBits(sim);
   a.cx = (real_t)(0.5 * box[0]); a.cy = (real_t)(0.5 * box[1]); a.cz = (real_t)(0.5 * box[2]);
   a.partial = sim->fdotrBuf;
   hipLaunchKernelGGL(Fdotr_atoms, atomsGrid, dim3(256), 0, st, a);
   FdotrFaceArgs v;
   v.rx = sim->atoms.r.x; v.ry = sim->atoms.r.y; v.rz = sim->atoms.r.z;
   v.nAtoms = sim->boxes.nAtoms; v.rows = sim->fdotrRows; v.nRows = sim->fdotrNRows; v.cap = sim->maxAtoms;
   v.lx = (real_t)box[0]; v.ly = (real_t)box[1]; v.lz = (real_t)box[2];
   v.partial = sim->fdotrBuf + (size_t)atomsGrid.x * VIRIAL_N;
   withPairFunction(sim, [&](auto p, real_t rc2) {
      v.rc2 = rc2;
      hipLaunchKernelGGL(Fdotr_face<decltype(p)>, dim3(FDOTR_FACE_BLOCKS), dim3(256), 0, st, v, p);
   });
   hipLaunchKernelGGL(Virial_Final, dim3(1), dim3(256), 0, st, sim->fdotrBuf, nPartial, out);
   LAUNCH_CHECK();
   double h[VIRIAL_N];
   HIP_CHECK(hipMemcpyAsync(h, out, sizeof h, hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
   for (int c = 0; c < VIRIAL_N; ++c) out12[c] = (real_t)h[c];
}

// Not in the reference: the pair-distance histogram (rdf_kernels.h).  One instance for every potential and method: it reads positions and cells only
extern "C" void computePairHistogram(SimGpu* sim, int nBins, real_t rMax, uint64_t* outCounts)
{
   hipStream_t st = analysisStream(sim);
   if (nBins < 1 || nBins > PAIRHIST_MAX_BINS) { fprintf(stderr, "computePairHistogram: %d bins (1..%d)\n", nBins, PAIRHIST_MAX_BINS); exit(-1); }
   if (nBins > sim->pairHistCap) {
      if (sim->pairHistBuf) { HIP_CHECK(hipStreamSynchronize(st)); HIP_CHECK(hipFree(sim->pairHistBuf)); }
      sim->pairHistBuf = dalloc<unsigned long long>((size_t)nBins, false);
      sim->pairHistCap = nBins;
   }
   PairHistArgs v;
   fillStencilArgs(v, sim);
   v.nBins = nBins; v.rMax2 = rMax * rMax; v.invDr = (real_t)nBins / rMax;
   v.counts = sim->pairHistBuf;
   const size_t lds = (size_t)4 * nBins * sizeof(unsigned);      // one copy per wave
   // what a workgroup can add to one 32-bit LDS counter stays below 2^32 (rdf_kernels.h); the grid does not show in a sum of integers
   const long nWork = (long)v.nLocalBoxes * v.chunks;
   int grid = PAIRHIST_BLOCKS;
   while ((double)((nWork + grid - 1) / grid) * WAVE * 27.0 * v.cap >= 4.0e9) grid *= 2;
   allowDynamicLds((const void*)PairHist_thread_atom, lds);
   HIP_CHECK(hipMemsetAsync(sim->pairHistBuf, 0, (size_t)nBins * sizeof(unsigned long long), st));
   hipLaunchKernelGGL(PairHist_thread_atom, dim3(grid), dim3(256), lds, st, v);
   LAUNCH_CHECK();
   HIP_CHECK(hipMemcpyAsync(outCounts, sim->pairHistBuf, (size_t)nBins * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// Not in the reference: the centro-symmetry parameter and the coordination number of every local atom (csp_kernels.h).  One instance for every
// potential and method: it reads positions and cells only.  The two per-slot buffers are allocated by the first call.
extern "C" void computeCentroSymmetry(SimGpu* sim, real_t rCoord, real_t* outCspBySlot, int* outCoordBySlot)
{
   hipStream_t st = analysisStream(sim);
   const real_t cutoff = pairCutoff(sim);
   if (!(rCoord > R(0.0)) || rCoord > cutoff) { fprintf(stderr, "computeCentroSymmetry: rCoord %g outside (0, cutoff = %g]\n", (double)rCoord, (double)cutoff); exit(-1); }
   refuseSlotsBeyondInt(sim, "computeCentroSymmetry");
   const size_t nSlots = localSlots(sim);
   if (!sim->cspBuf) {
      sim->cspBuf = dalloc<real_t>(nSlots);
      sim->cspCoordBuf = dalloc<int>(nSlots);
   }
   CentroSymArgs v;
   fillStencilArgs(v, sim);
   v.rc2 = cutoff * cutoff; v.rCoord2 = rCoord * rCoord;
   v.csp = sim->cspBuf; v.coord = sim->cspCoordBuf;
   hipLaunchKernelGGL(CentroSym_thread_atom, dim3(CSP_BLOCKS), dim3(256), 0, st, v);
   LAUNCH_CHECK();
   HIP_CHECK(hipMemcpyAsync(outCspBySlot, sim->cspBuf, nSlots * sizeof(real_t), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipMemcpyAsync(outCoordBySlot, sim->cspCoordBuf, nSlots * sizeof(int), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// Not in the reference: adaptive common neighbour analysis, the structure type of every local atom (cna_kernels.h).  One instance for every potential
// and method, as computeCentroSymmetry, whose walk it shares.  The per-slot buffer is allocated by the first call.
extern "C" void computeCommonNeighbors(SimGpu* sim, int* outTypeBySlot)
{
   hipStream_t st = analysisStream(sim);
   const real_t cutoff = pairCutoff(sim);
   refuseSlotsBeyondInt(sim, "computeCommonNeighbors");
   const size_t nSlots = localSlots(sim);
   if (!sim->cnaBuf) sim->cnaBuf = dalloc<int>(nSlots);
   CnaArgs v;
   fillStencilArgs(v, sim);
   v.rc2 = cutoff * cutoff;
   v.type = sim->cnaBuf;
   hipLaunchKernelGGL(Cna_thread_atom, dim3(CNA_BLOCKS), dim3(256), 0, st, v);
   LAUNCH_CHECK();
   HIP_CHECK(hipMemcpyAsync(outTypeBySlot, sim->cnaBuf, nSlots * sizeof(int), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// Not in the reference: the per-atom virial stress (stress_kernels.h), one kernel instance per pair function of the force paths, as computeVirial.
// The six planes and the rows of the summary are allocated by the first call.
extern "C" void computeAtomStress(SimGpu* sim, int withKinetic, real_t* outBySlot6)
{
   hipStream_t st = analysisStream(sim);
   const size_t nSlots = localSlots(sim);
   if (!sim->stressBuf) {
      sim->stressBuf = dalloc<real_t>(6 * nSlots);
      sim->stressSumBuf = dalloc<double>((size_t)(ATOMSTRESS_SUM_BLOCKS + 1) * ATOMSTRESS_SUM_N, false);
   }
   AtomStressArgs v;
   fillStencilArgs(v, sim);
   v.px = sim->atoms.p.x; v.py = sim->atoms.p.y; v.pz = sim->atoms.p.z;
   v.iSpecies = sim->atoms.iSpecies; v.speciesMass = sim->species_mass;
   v.withKinetic = withKinetic != 0;
   v.plane = nSlots;
   withPairFunction(sim, [&](auto p, real_t rc2) {
      v.rc2 = rc2;
      hipLaunchKernelGGL(AtomStress_thread_atom<decltype(p)>, dim3(ATOMSTRESS_BLOCKS), dim3(256), 0, st, v, p, sim->stressBuf);
   });
   LAUNCH_CHECK();
   if (outBySlot6) HIP_CHECK(hipMemcpyAsync(outBySlot6, sim->stressBuf, 6 * nSlots * sizeof(real_t), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// The two stages of a summary (slot_summary.h) over the planes a compute... call has left on the device: stage 1 into the nRows rows of `rows`, stage 2
// into the row behind them, whose n doubles come back, not the planes
typedef void (*SummaryStage1)(const real_t*, size_t, const int*, const int*, int, double, double*);
typedef void (*SummaryStage2)(const double*, int, double*);
static void launchSummary(SimGpu* sim, SummaryStage1 stage1, SummaryStage2 stage2, const real_t* planes, double param, double* rows, int nRows, int n, double* out)
{
   hipStream_t st = analysisStream(sim);
   double* final = rows + (size_t)nRows * n;
   hipLaunchKernelGGL(stage1, dim3(nRows), dim3(256), 0, st, planes, localSlots(sim), sim->boxes.nAtoms, sim->atoms.gid, sim->maxAtoms, param, rows);
   hipLaunchKernelGGL(stage2, dim3(1), dim3(256), 0, st, rows, nRows, final);
   LAUNCH_CHECK();
   HIP_CHECK(hipMemcpyAsync(out, final, n * sizeof(double), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// Not in the reference: the printed-step figures of the planes computeAtomStress has left on the device (stress_kernels.h): 7 doubles
extern "C" void computeAtomStressSummary(SimGpu* sim, double atomVolume, double* out)
{
   if (!sim->stressBuf) { fprintf(stderr, "computeAtomStressSummary: no computeAtomStress call before it\n"); exit(-1); }
   launchSummary(sim, AtomStress_Summary, AtomStress_SummaryFinal, sim->stressBuf, 1.0 / atomVolume, sim->stressSumBuf, ATOMSTRESS_SUM_BLOCKS, ATOMSTRESS_SUM_N, out);
}

// Not in the reference: the per-atom heat flux (heatflux_kernels.h), one kernel instance per pair function of the force paths and per output, as computeVirial.
// outBySlot9: the nine planes are stored and copied; else, out9: the sampled path, nine sums of this rank's atoms through the rows, nothing per atom written.
// The planes and the rows are allocated by the first call that needs them.
extern "C" void computeHeatFlux(SimGpu* sim, real_t* outBySlot9, double* out9)
{
   hipStream_t st = analysisStream(sim);
   const size_t nSlots = localSlots(sim);
   HeatFluxArgs v;
   fillStencilArgs(v, sim);
   v.px = sim->atoms.p.x; v.py = sim->atoms.p.y; v.pz = sim->atoms.p.z;
   v.e = sim->atoms.e;
   v.iSpecies = sim->atoms.iSpecies; v.speciesMass = sim->species_mass;
   v.plane = nSlots;
   if (outBySlot9) {
      if (!sim->heatFluxBuf) sim->heatFluxBuf = dalloc<real_t>(HEATFLUX_N * nSlots);
      withPairFunction(sim, [&](auto p, real_t rc2) {
         v.rc2 = rc2;
         hipLaunchKernelGGL((HeatFlux_thread_atom<decltype(p), true>), dim3(HEATFLUX_BLOCKS), dim3(256), 0, st, v, p, sim->heatFluxBuf, (double*)nullptr);
      });
      LAUNCH_CHECK();
      HIP_CHECK(hipMemcpyAsync(outBySlot9, sim->heatFluxBuf, HEATFLUX_N * nSlots * sizeof(real_t), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
   }
   if (out9) {
      if (!sim->heatFluxSumBuf) sim->heatFluxSumBuf = dalloc<double>((size_t)(HEATFLUX_BLOCKS + 1) * HEATFLUX_N, false);
      double* final = sim->heatFluxSumBuf + (size_t)HEATFLUX_BLOCKS * HEATFLUX_N;
      withPairFunction(sim, [&](auto p, real_t rc2) {
         v.rc2 = rc2;
         hipLaunchKernelGGL((HeatFlux_thread_atom<decltype(p), false>), dim3(HEATFLUX_BLOCKS), dim3(256), 0, st, v, p, (real_t*)nullptr, sim->heatFluxSumBuf);
      });
      hipLaunchKernelGGL(HeatFlux_Final, dim3(1), dim3(256), 0, st, sim->heatFluxSumBuf, HEATFLUX_BLOCKS, final);
      LAUNCH_CHECK();
      HIP_CHECK(hipMemcpyAsync(out9, final, HEATFLUX_N * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
   }
}

// Not in the reference: the reference snapshot of the per-atom strain (strain_kernels.h).  on: one 32-byte record of doubles per global atom id, zeroed, then
// the positions of this rank's local atoms at their gids (taken again when it is already on); the host adds the ranks' tables and uploads the sum into
// strainRefBuf.  off: the table and the planes of computeAtomStrain are freed.  1 and no reference when the device cannot give the memory.
static void freeStrainPlanes(SimGpu* sim)
{
   if (sim->strainBuf) { HIP_CHECK(hipFree(sim->strainBuf)); HIP_CHECK(hipFree(sim->strainCountBuf)); HIP_CHECK(hipFree(sim->strainSumBuf)); }
   sim->strainBuf = nullptr; sim->strainCountBuf = nullptr; sim->strainSumBuf = nullptr;
}

extern "C" int comdStrainReferenceGpu(SimGpu* sim, int nGlobal, int on)
{
   hipStream_t st = analysisStream(sim);
   if (!on || nGlobal != sim->strainRefN) {
      if (sim->strainRefBuf || sim->strainBuf) HIP_CHECK(hipStreamSynchronize(st));
      if (sim->strainRefBuf) HIP_CHECK(hipFree(sim->strainRefBuf));
      sim->strainRefBuf = nullptr; sim->strainRefN = 0;
      freeStrainPlanes(sim);
      if (!on) return 0;
   }
   if (nGlobal < 1) return 1;
   if (!sim->strainRefBuf) {
      void* d = nullptr;
      if (hipMalloc(&d, (size_t)nGlobal * 4 * sizeof(double)) != hipSuccess) {
         (void)hipGetLastError();
         fprintf(stderr, "comdStrainReferenceGpu: rank %d: no device memory for %d records of 32 bytes (%.1f MB): no reference\n",
                 g_rank, nGlobal, nGlobal * 32.0 / 1048576.0);
         return 1;
      }
      sim->strainRefBuf = (double*)d; sim->strainRefN = nGlobal;
   }
   const size_t nSlots = localSlots(sim);
   HIP_CHECK(hipMemsetAsync(sim->strainRefBuf, 0, (size_t)nGlobal * 4 * sizeof(double), st));
   const size_t blocks = (nSlots + 255) / 256;
   hipLaunchKernelGGL(StrainReference_Store, dim3((unsigned)(blocks < 4096 ? (blocks ? blocks : 1) : 4096)), dim3(256), 0, st, sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z,
                      sim->boxes.nAtoms, sim->atoms.gid, sim->maxAtoms, nSlots, nGlobal, sim->strainRefBuf);
   LAUNCH_CHECK();
   HIP_CHECK(hipStreamSynchronize(st));
   return 0;
}

// Not in the reference: the per-atom strain tensor and D^2min against the reference table (strain_kernels.h).  One instance for every potential and
// method: it reads positions, gids and cells only.  The planes and the rows of the summary are allocated by the first call.
extern "C" void computeAtomStrain(SimGpu* sim, real_t rCut, real_t* outBySlot7, int* outCountBySlot)
{
   hipStream_t st = analysisStream(sim);
   const real_t cutoff = pairCutoff(sim);
   if (!sim->strainRefBuf) { fprintf(stderr, "computeAtomStrain: no reference (comdStrainReferenceGpu)\n"); exit(-1); }
   if (!(rCut > R(0.0)) || rCut > cutoff) { fprintf(stderr, "computeAtomStrain: rCut %g outside (0, cutoff = %g]\n", (double)rCut, (double)cutoff); exit(-1); }
   for (int a = 0; a < 3; ++a)
      if (!(sim->strainL[a] > 0.0)) { fprintf(stderr, "computeAtomStrain: sim->strainL[%d] = %g: set it to the current global box before the call\n", a, sim->strainL[a]); exit(-1); }
   const size_t nSlots = localSlots(sim);
   if (!sim->strainBuf) {
      sim->strainBuf = dalloc<real_t>(ATOMSTRAIN_PLANES * nSlots);
      sim->strainCountBuf = dalloc<int>(nSlots);
      sim->strainSumBuf = dalloc<double>((size_t)(ATOMSTRAIN_SUM_BLOCKS + 1) * ATOMSTRAIN_SUM_N, false);
   }
   AtomStrainArgs v;
   fillStencilArgs(v, sim);
   v.gid = sim->atoms.gid; v.ref = sim->strainRefBuf; v.nRef = sim->strainRefN;
   v.rs2 = rCut * rCut;
   v.L0x = sim->strainL0[0]; v.L0y = sim->strainL0[1]; v.L0z = sim->strainL0[2];
   v.sx = sim->strainL0[0] / sim->strainL[0]; v.sy = sim->strainL0[1] / sim->strainL[1]; v.sz = sim->strainL0[2] / sim->strainL[2];
   v.plane = nSlots;
   hipLaunchKernelGGL(AtomStrain_thread_atom, dim3(ATOMSTRAIN_BLOCKS), dim3(256), 0, st, v, sim->strainBuf, sim->strainCountBuf);
   LAUNCH_CHECK();
   if (outBySlot7) HIP_CHECK(hipMemcpyAsync(outBySlot7, sim->strainBuf, ATOMSTRAIN_PLANES * nSlots * sizeof(real_t), hipMemcpyDeviceToHost, st));
   if (outCountBySlot) HIP_CHECK(hipMemcpyAsync(outCountBySlot, sim->strainCountBuf, nSlots * sizeof(int), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// Not in the reference: the printed-step figures of the planes computeAtomStrain has left on the device (strain_kernels.h): 9 doubles
extern "C" void computeAtomStrainSummary(SimGpu* sim, double threshold, double* out)
{
   if (!sim->strainBuf) { fprintf(stderr, "computeAtomStrainSummary: no computeAtomStrain call before it\n"); exit(-1); }
   launchSummary(sim, AtomStrain_Summary, AtomStrain_SummaryFinal, sim->strainBuf, threshold, sim->strainSumBuf, ATOMSTRAIN_SUM_BLOCKS, ATOMSTRAIN_SUM_N, out);
}

// Not in the reference: Steinhardt's bond-orientational order q4, q6, w4, w6 of every local atom (steinhardt_kernels.h).  One instance for every potential
// and method, as computeCentroSymmetry, whose walk it shares.  The four planes and the rows of the summary are allocated by the first call.
extern "C" void computeSteinhardt(SimGpu* sim, real_t* outBySlot4)
{
   hipStream_t st = analysisStream(sim);
   const real_t cutoff = pairCutoff(sim);
   refuseSlotsBeyondInt(sim, "computeSteinhardt");
   const size_t nSlots = localSlots(sim);
   if (!sim->steinhardtBuf) {
      sim->steinhardtBuf = dalloc<real_t>(STEINHARDT_PLANES * nSlots);
      sim->steinhardtSumBuf = dalloc<double>((size_t)(STEINHARDT_SUM_BLOCKS + 1) * STEINHARDT_SUM_N, false);
   }
   SteinhardtArgs v;
   fillStencilArgs(v, sim);
   v.rc2 = cutoff * cutoff;
   v.plane = nSlots;
   hipLaunchKernelGGL(Steinhardt_thread_atom, dim3(STEINHARDT_BLOCKS), dim3(256), 0, st, v, sim->steinhardtBuf);
   LAUNCH_CHECK();
   if (outBySlot4) HIP_CHECK(hipMemcpyAsync(outBySlot4, sim->steinhardtBuf, STEINHARDT_PLANES * nSlots * sizeof(real_t), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// Not in the reference: the printed-step figures of the planes computeSteinhardt has left on the device (steinhardt_kernels.h): 10 doubles
extern "C" void computeSteinhardtSummary(SimGpu* sim, double threshold, double* out)
{
   if (!sim->steinhardtBuf) { fprintf(stderr, "computeSteinhardtSummary: no computeSteinhardt call before it\n"); exit(-1); }
   launchSummary(sim, Steinhardt_Summary, Steinhardt_SummaryFinal, sim->steinhardtBuf, threshold, sim->steinhardtSumBuf, STEINHARDT_SUM_BLOCKS, STEINHARDT_SUM_N, out);
}

// the second-derivative sibling (born_kernels.h) of a pair functor of withPairFunction
static BornLj bornPairOf(const SimGpu*, const VirialLj& p) { BornLj b; b.s6x14 = R(7.0) * p.a.s6x2; b.fs = p.scale(); return b; }
static BornLjTable bornPairOf(const SimGpu*, const VirialLjTable& p) { BornLjTable b; b.t = p.t; return b; }
template <bool SPLINE>
static BornEam<SPLINE> bornPairOf(const SimGpu* sim, const VirialEam<SPLINE>& p)
{
   BornEam<SPLINE> b;
   b.phi = p.phi; b.rho = p.rho; b.f = sim->eam_pot.f; b.phiS = p.phiS; b.rhoS = p.rhoS;
   b.dfEmbed = p.dfEmbed; b.rhobar = sim->eam_pot.rhobar; b.dfi = R(0.0); b.d2fi = R(0.0);
   return b;
}

// Not in the reference: the Born matrix (born_kernels.h), one kernel instance per pair function of the force paths, as computeVirial.  The rows are
// allocated by the first call.
extern "C" void computeBornMatrix(SimGpu* sim, double* out21)
{
   hipStream_t st = analysisStream(sim);
   if (!sim->bornBuf) sim->bornBuf = dalloc<double>((size_t)(BORN_BLOCKS + 1) * BORN_N, false);
   BornArgs v;
   fillStencilArgs(v, sim);
   double* out = sim->bornBuf + (size_t)BORN_BLOCKS * BORN_N;
   withPairFunction(sim, [&](auto p, real_t rc2) {
      v.rc2 = rc2;
      auto b = bornPairOf(sim, p);
      hipLaunchKernelGGL(BornMatrix_thread_atom<decltype(b)>, dim3(BORN_BLOCKS), dim3(256), 0, st, v, b, sim->bornBuf);
   });
   hipLaunchKernelGGL(BornMatrix_Final, dim3(1), dim3(256), 0, st, (const double*)sim->bornBuf, BORN_BLOCKS, out);
   LAUNCH_CHECK();
   HIP_CHECK(hipMemcpyAsync(out21, out, BORN_N * sizeof(double), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// Not in the reference: displacement tracking for the mean-squared displacement (msd_kernels.h).  on: one zeroed 32-byte record per global atom id,
// which the drift kernels of this simulation add into from now on (already on: zeroed again, the origin becomes "now"); off: the memory is
// freed.  1 and nothing tracked when the device cannot give the memory.
extern "C" int comdTrackDisplacementGpu(SimGpu* sim, int nGlobal, int on)
{
   hipStream_t st = S(sim->boundary_stream);
   if (!on || nGlobal != sim->dispN) {
      if (sim->dispBuf) {
         HIP_CHECK(hipStreamSynchronize(st));               // the last drift kernel has written its records
         HIP_CHECK(hipFree(sim->dispBuf)); HIP_CHECK(hipFree(sim->dispSumBuf));
      }
      sim->dispBuf = nullptr; sim->dispSumBuf = nullptr; sim->dispN = 0;
      if (!on) return 0;
   }
   if (nGlobal < 1) return 1;
   if (!sim->dispBuf) {
      void *d = nullptr, *p = nullptr;
      if (hipMalloc(&d, (size_t)nGlobal * 4 * sizeof(long long)) != hipSuccess
          || hipMalloc(&p, (size_t)(MSD_BLOCKS + 1) * MSD_N * sizeof(double)) != hipSuccess) {
         (void)hipGetLastError();
         if (d) (void)hipFree(d);
         fprintf(stderr, "comdTrackDisplacementGpu: rank %d: no device memory for %d records of 32 bytes (%.1f MB): not tracking\n",
                 g_rank, nGlobal, nGlobal * 32.0 / 1048576.0);
         return 1;
      }
      sim->dispBuf = (int64_t*)d; sim->dispSumBuf = (double*)p; sim->dispN = nGlobal;
   }
   HIP_CHECK(hipMemsetAsync(sim->dispBuf, 0, (size_t)nGlobal * 4 * sizeof(long long), st));      // behind the drifts already launched
   HIP_CHECK(hipStreamSynchronize(st));
   return 0;
}

// Not in the reference: {sum dx, dy, dz, sum dx^2, dy^2, dz^2} (Angstroms, double in both builds) over THIS rank's records
extern "C" void computeDisplacementSums(SimGpu* sim, double* out6)
{
   hipStream_t st = S(sim->boundary_stream);
   if (!sim->dispBuf) { fprintf(stderr, "computeDisplacementSums: displacements are not tracked\n"); exit(-1); }
   int blocks = ceilDiv(sim->dispN, 256);
   if (blocks > MSD_BLOCKS) blocks = MSD_BLOCKS;
   double* out = sim->dispSumBuf + (size_t)MSD_BLOCKS * MSD_N;
   hipLaunchKernelGGL(ReduceDisplacementPartial, dim3(blocks), dim3(256), 0, st, (const long long*)sim->dispBuf, sim->dispN, sim->dispSumBuf);
   hipLaunchKernelGGL(ReduceDisplacementFinal, dim3(1), dim3(256), 0, st, sim->dispSumBuf, blocks, out);
   LAUNCH_CHECK();
   HIP_CHECK(hipMemcpyAsync(out6, out, MSD_N * sizeof(double), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// Not in the reference: THIS rank's raw records, [nGlobal][4] int64 {dx, dy, dz, spare} in units of 2^-32 Angstroms
extern "C" void comdCopyDisplacementsGpu(SimGpu* sim, int64_t* out)
{
   hipStream_t st = S(sim->boundary_stream);
   if (!sim->dispBuf) { fprintf(stderr, "comdCopyDisplacementsGpu: displacements are not tracked\n"); exit(-1); }
   HIP_CHECK(hipMemcpyAsync(out, sim->dispBuf, (size_t)sim->dispN * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// Not in the reference: the slab profile (profile_kernels.h).  One instance for every potential and method: it reads r, p, e and the cell tables only
extern "C" void computeSlabProfile(SimGpu* sim, int axis, int nBins, double extent, int64_t* out6xN)
{
   hipStream_t st = analysisStream(sim);
   if (axis < 0 || axis > 2 || nBins < 1 || nBins > PROFILE_MAX_BINS || !(extent > 0.0)) {
      fprintf(stderr, "computeSlabProfile: axis %d (0..2), %d bins (1..%d), extent %g\n", axis, nBins, PROFILE_MAX_BINS, extent); exit(-1);
   }
   if (nBins > sim->profileCap) {
      if (sim->profileBuf) { HIP_CHECK(hipStreamSynchronize(st)); HIP_CHECK(hipFree(sim->profileBuf)); }
      sim->profileBuf = (uint64_t*)dalloc<unsigned long long>((size_t)PROFILE_PLANES * nBins, false);
      sim->profileCap = nBins;
   }
   ProfileArgs v;
   v.ra = axis == 0 ? sim->atoms.r.x : axis == 1 ? sim->atoms.r.y : sim->atoms.r.z;
   v.px = sim->atoms.p.x; v.py = sim->atoms.p.y; v.pz = sim->atoms.p.z; v.e = sim->atoms.e;
   v.iSpecies = sim->atoms.iSpecies; v.speciesMass = sim->species_mass; v.nAtoms = sim->boxes.nAtoms;
   v.nLocalBoxes = sim->boxes.nLocalBoxes; v.cap = sim->maxAtoms; v.laneBits = integratorLaneBits(sim); v.nBins = nBins;
   v.invWidth = (real_t)nBins / (real_t)extent;
   v.out = (unsigned long long*)sim->profileBuf;
   const size_t bytes = (size_t)PROFILE_PLANES * nBins * sizeof(unsigned long long);
   allowDynamicLds((const void*)Profile_slabs, bytes);
   HIP_CHECK(hipMemsetAsync(sim->profileBuf, 0, bytes, st));
   hipLaunchKernelGGL(Profile_slabs, integratorGrid(sim), dim3(256), bytes, st, v);
   LAUNCH_CHECK();
   HIP_CHECK(hipMemcpyAsync(out6xN, sim->profileBuf, bytes, hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// Not in the reference: the candidates of a Mueller-Plathe exchange (mp_kernels.h), MP_select's records of all workgroups, then MP_merge's two lists
extern "C" void computeMullerPlatheCandidates(SimGpu* sim, int axis, int nBins, double extent, int k, double* out2xKx6)
{
   hipStream_t st = analysisStream(sim);
   if (axis < 0 || axis > 2 || nBins < 2 || nBins > PROFILE_MAX_BINS || (nBins & 1) || k < 1 || k > MP_MAX_SWAPS || !(extent > 0.0)) {
      fprintf(stderr, "computeMullerPlatheCandidates: axis %d (0..2), %d bins (even, 2..%d), %d swaps (1..%d), extent %g\n", axis, nBins, PROFILE_MAX_BINS, k, MP_MAX_SWAPS, extent);
      exit(-1);
   }
   const size_t partial = (size_t)2 * MP_BLOCKS * MP_MAX_SWAPS * MP_RECORD, merged = (size_t)2 * MP_MAX_SWAPS * MP_RECORD;
   if (!sim->mpBuf) sim->mpBuf = dalloc<double>(partial + merged, false);
   MpSelectArgs v;
   v.ra = axis == 0 ? sim->atoms.r.x : axis == 1 ? sim->atoms.r.y : sim->atoms.r.z;
   v.px = sim->atoms.p.x; v.py = sim->atoms.p.y; v.pz = sim->atoms.p.z; v.gid = sim->atoms.gid;
   v.iSpecies = sim->atoms.iSpecies; v.speciesMass = sim->species_mass; v.nAtoms = sim->boxes.nAtoms;
   v.nLocalBoxes = sim->boxes.nLocalBoxes; v.cap = sim->maxAtoms; v.laneBits = integratorLaneBits(sim); v.nBins = nBins; v.k = k;
   v.invWidth = (real_t)nBins / (real_t)extent;
   v.partial = sim->mpBuf;
   double* out = sim->mpBuf + partial;
   hipLaunchKernelGGL(MP_select, dim3(MP_BLOCKS), dim3(256), 0, st, v);
   hipLaunchKernelGGL(MP_merge, dim3(2), dim3(256), 0, st, (const double*)sim->mpBuf, MP_BLOCKS, k, out);
   LAUNCH_CHECK();
   HIP_CHECK(hipMemcpyAsync(out2xKx6, out, (size_t)2 * k * MP_RECORD * sizeof(double), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}

// The exchange: every slot is checked here, the kernel trusts the rows
extern "C" void comdMullerPlatheApplyGpu(SimGpu* sim, int n, const long long* slots, const real_t* p3)
{
   hipStream_t st = analysisStream(sim);
   if (n < 0 || n > 2 * MP_MAX_SWAPS) { fprintf(stderr, "comdMullerPlatheApplyGpu: %d rows (0..%d)\n", n, 2 * MP_MAX_SWAPS); exit(-1); }
   const long long nSlots = (long long)localSlots(sim);
   for (int i = 0; i < n; ++i)
      if (slots[i] < 0 || slots[i] >= nSlots) { fprintf(stderr, "comdMullerPlatheApplyGpu: row %d: slot %lld is not a local slot (0..%lld)\n", i, slots[i], nSlots - 1); exit(-1); }
   if (n == 0) return;
   const size_t slotBytes = (size_t)2 * MP_MAX_SWAPS * sizeof(long long);
   if (!sim->mpRows) sim->mpRows = dalloc<char>(slotBytes + (size_t)2 * MP_MAX_SWAPS * 3 * sizeof(real_t), false);
   long long* dSlots = (long long*)sim->mpRows;
   real_t* dP = (real_t*)((char*)sim->mpRows + slotBytes);
   HIP_CHECK(hipMemcpyAsync(dSlots, slots, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, st));
   HIP_CHECK(hipMemcpyAsync(dP, p3, (size_t)3 * n * sizeof(real_t), hipMemcpyHostToDevice, st));
   hipLaunchKernelGGL(MP_apply, dim3(1), dim3(128), 0, st, n, (const long long*)dSlots, (const real_t*)dP, sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z);
   LAUNCH_CHECK();
   HIP_CHECK(hipStreamSynchronize(st));
}

// Not in the reference: the density amplitudes of the structure factor (sk_kernels.h).  One instance for every potential and method: it reads r and the cell tables only
extern "C" void computeStructureFactor(SimGpu* sim, int M, const int* stride3, const double* extent3, double* outKx2)
{
   hipStream_t st = analysisStream(sim);
   bool ok = M >= 1 && M <= SK_MAX_M;
   for (int a = 0; a < 3; ++a) ok = ok && stride3[a] >= 1 && (long)stride3[a] * M <= SK_MAX_HM && extent3[a] > 0.0;
   if (!ok) {
      fprintf(stderr, "computeStructureFactor: M %d (1..%d), strides %d %d %d (>= 1, stride M <= %d), extents %g %g %g\n", M, SK_MAX_M, stride3[0], stride3[1], stride3[2], SK_MAX_HM,
              extent3[0], extent3[1], extent3[2]);
      exit(-1);
   }
   SkArgs v;
   v.rx = sim->atoms.r.x; v.ry = sim->atoms.r.y; v.rz = sim->atoms.r.z; v.nAtoms = sim->boxes.nAtoms;
   v.nLocalBoxes = sim->boxes.nLocalBoxes; v.cap = sim->maxAtoms;
   v.M = M; v.W = 2 * M + 1; v.lbNeg = ceilDiv(M, SK_LB); v.nLB = v.lbNeg + M / SK_LB + 1;
   v.nItems = (M + 1) * v.W * v.nLB;
   v.sx = stride3[0]; v.sy = stride3[1]; v.sz = stride3[2];
   v.Lx = extent3[0]; v.Ly = extent3[1]; v.Lz = extent3[2];
   const int nTiles = ceilDiv(v.nItems, 256);
   int tableMax = 0;
   for (int tile = 0; tile < nTiles; ++tile) {
      const SkTile t = skTileOf(tile, v.nItems, v.nLB, v.W, M);
      if (t.nH + t.nKa > tableMax) tableMax = t.nH + t.nKa;
   }
   auto ldsOf = [&](int batch) { return (size_t)3 * batch * sizeof(double) + (size_t)batch * (tableMax + v.nLB + 1) * sizeof(real2); };
   v.batch = ldsOf(SK_BATCH_MAX) <= SK_LDS_FOR_64 ? SK_BATCH_MAX : SK_BATCH_MAX / 2;
   const size_t lds = ldsOf(v.batch);
   if (lds > 65536) { fprintf(stderr, "computeStructureFactor: %zu bytes of LDS\n", lds); exit(-1); }
   // the chunks: a few workgroups per CU in all; one when the tiles alone fill the device
   int dev = 0, cus = 0;
   HIP_CHECK(hipGetDevice(&dev));
   HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
   const int nLocal = v.nLocalBoxes > 0 ? v.nLocalBoxes : 1;
   int chunks = tuningOf(sim).skChunks ? tuningOf(sim).skChunks : ceilDiv((long)4 * cus, nTiles);
   if (chunks > nLocal) chunks = nLocal;
   if (chunks > 65535) chunks = 65535;
   if (chunks < 1) chunks = 1;
   v.cellsPerChunk = ceilDiv(nLocal, chunks);
   chunks = ceilDiv(nLocal, v.cellsPerChunk);
   const size_t n = (size_t)2 * (M + 1) * v.W * v.W, need = ((size_t)chunks + 1) * n;
   if (need > sim->skCap) {
      if (sim->skBuf) { HIP_CHECK(hipStreamSynchronize(st)); HIP_CHECK(hipFree(sim->skBuf)); }
      sim->skBuf = dalloc<double>(need, false);
      sim->skCap = need;
   }
   v.partial = sim->skBuf;
   double* out = sim->skBuf + (size_t)chunks * n;
   allowDynamicLds((const void*)SK_amplitudes, lds);
   hipLaunchKernelGGL(SK_amplitudes, dim3(nTiles, chunks), dim3(256), lds, st, v);
   hipLaunchKernelGGL(SK_sum, dim3(ceilDiv((long)n, 256)), dim3(256), 0, st, (const double*)sim->skBuf, chunks, n, out);
   LAUNCH_CHECK();
   HIP_CHECK(hipMemcpyAsync(outKx2, out, n * sizeof(double), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
}
