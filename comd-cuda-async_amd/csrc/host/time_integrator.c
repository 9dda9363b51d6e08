/* time_integrator.c -- velocity-Verlet driver: half kick, drift, redistribute, force, half kick
 * (timestep.c:48-100), computeForce through the potential's function pointer (:102-105), the energy
 * reduction (:184-197) and the per-step atom redistribution (:222-276).  Every phase is a call into
 * include/comd_hip.h; the only blocking device round-trip per step on one rank is none at all
 * (the reference has >= 20) -- energies are fetched every printRate steps. */
#include "comd_host.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

static void advanceVelocity(SimFlat* s, real_t dt) { advanceVelocityGpu(&s->gpu, dt); }

/* --langevin (not in the reference): BAOAB, the O update between the two half drifts of each step (hip/langevin_kernels.h).  c1, c2 from
 * this call's dt, in double */
typedef struct { int on; real_t c1, c2, kT; uint64_t seed; } Langevin;
static Langevin langevinOf(const SimFlat* s, real_t dt)
{
   Langevin l = { s->langevin, 0, 0, 0, s->langevinSeed };
   if (l.on) {
      const double c1 = exp(-(double)dt / s->langevinDamp);
      l.c1 = (real_t)c1; l.c2 = (real_t)sqrt(1.0 - c1 * c1); l.kT = (real_t)(kB_eV * s->langevinTemp);
   }
   return l;
}

/* ---- box deformation (not in the reference; comd_host.h) ---- */
static void extentsAt(const SimFlat* s, double t, double L[3])
{
   for (int a = 0; a < 3; ++a) L[a] = s->box0[a] * (1.0 + (s->deformEpsBase[a] + s->erate[a] * t / 1000.0));
}

/* One step's strain: the box is set from box0 and the strained time, never by multiplying up, so it is a pure function of the steps taken; the kernel gets
 * L_new / L_old.  A box the grid cannot follow ends the run here, before anything is launched. */
static void deformStep(SimFlat* s, real_t dt)
{
   double L[3];
   s->deformTime += (double)dt;
   extentsAt(s, s->deformTime, L);
   if (comdSetBox(s, L) != 0) {
      if (printRank())
         printf("Error: at step %llu the box [ %g, %g, %g ] would make a link cell narrower than the %g Angstroms the grid was built for (or is not positive); "
                "re-gridding is not implemented.\n", (unsigned long long)s->stepCount, L[0], L[1], L[2], (double)s->boxes->builtRange);
      fflush(stdout);
      exit(-1);
   }
   extentsAt(s, s->deformTime + (double)dt, s->nextExtent);
   deformListBudget(s);
}

/* Verlet lists under a changing box.  A pair further apart than rc + skin at the build is, after the box has been compressed to the share
 * Lambda_a of its extent at the build, still further apart than (1 - e_c) (rc + skin) before any non-affine motion, e_c = max_a max(0, 1 - Lambda_a); it stays
 * outside rc while every atom's non-affine displacement -- what the drift kernels measure against the remapped snapshot -- is below (skin - e_c (rc + skin)) / 2.
 * The drift kernel of a step runs before the remap of the next, so e_c is taken over the current box and the one the coming step will set.  Below half of the
 * skin's own skin / 2 the lists are built again. */
void deformListBudget(SimFlat* s)
{
   if (!s->useNL || !s->gpu.boxes.nAtoms) return;
   double ec = 0.0;
   for (int a = 0; a < 3; ++a) {
      const double now = (double)s->domain->globalExtent[a], low = s->nextExtent[a] < now ? s->nextExtent[a] : now;
      const double e = 1.0 - low / s->listExtent[a];
      if (e > ec) ec = e;
   }
   const double skin = (double)s->skinDistance, budget = (skin - ec * ((double)s->pot->cutoff + skin)) / skin;
   if (budget < 0.5) neighborListForceRebuildGpu(&s->gpu.atoms.neighborList);
   comdSetListBudgetGpu(&s->gpu, budget < 0.5 ? 1.0 : budget);
}

int comdSetBox(SimFlat* s, const double L[3])
{
   Domain* dd = s->domain; LinkCell* ll = s->boxes;
   real_t ext[3]; double scale[3];
   for (int a = 0; a < 3; ++a) {
      if (!(L[a] > 0.0) || !(L[a] < 1e300)) return -1;
      ext[a] = (real_t)L[a];
      /* the cell width setDomainExtent and setLinkCellExtent would arrive at */
      const real_t localExtent = ext[a] / dd->procGrid[a];
      if (!(localExtent / (real_t)ll->gridSize[a] >= ll->builtRange)) return -1;
      scale[a] = (double)ext[a] / (double)dd->globalExtent[a];
   }
   setDomainExtent(dd, ext);
   setLinkCellExtent(ll, dd);
   if (s->atomExchange) haloSetBox(s->atomExchange, dd);
   if (s->positionExchange) haloSetBox(s->positionExchange, dd);
   if (s->cmdDoeam && ((EamPotential*)s->pot)->forceExchange) haloSetBox(((EamPotential*)s->pot)->forceExchange, dd);
   if (s->gpu.boxes.nAtoms) comdRemapBoxGpu(&s->gpu, scale, ll->localMin, ll->localMax, ll->boxSize, s->gpu.boundary_stream);
   for (int a = 0; a < 3; ++a) s->nextExtent[a] = (double)ext[a];
   s->boxChanged = 1;
   return 0;
}

int comdDeformTo(SimFlat* s, const double L[3])
{
   if (comdSetBox(s, L) != 0) return -1;
   if (!s->gpu.boxes.nAtoms) return 0;
   if (s->useNL) neighborListForceRebuildGpu(&s->gpu.atoms.neighborList);
   redistributeAtoms(s);
   computeForce(s);
   kineticEnergyGpu(s);
   return 0;
}

int comdSetStrainRate(SimFlat* s, const double r[3])
{
   const int on = r[0] != 0.0 || r[1] != 0.0 || r[2] != 0.0;
   for (int a = 0; a < 3; ++a) if (!(r[a] == r[a]) || !(fabs(r[a]) < 1e300)) return -1;
   if (on && s->gpuProfile) return -1;
   for (int a = 0; a < 3; ++a) {
      s->deformEpsBase[a] = (double)s->domain->globalExtent[a] / s->box0[a] - 1.0;
      s->erate[a] = r[a];
   }
   s->deformTime = 0.0;
   s->deform = on;
   for (int a = 0; a < 3; ++a) s->nextExtent[a] = (double)s->domain->globalExtent[a];
   deformListBudget(s);
   return 0;
}

void comdGetBox(SimFlat* s, double out[6])
{
   for (int a = 0; a < 3; ++a) { out[a] = (double)s->domain->globalExtent[a]; out[3 + a] = s->box0[a]; }
}

void comdLocalBounds(SimFlat* s, double out[6])
{
   for (int a = 0; a < 3; ++a) { out[a] = (double)s->domain->localMin[a]; out[3 + a] = (double)s->domain->localMax[a]; }
}

double timestep(SimFlat* s, int nSteps, real_t dt)
{
   const Langevin lv = langevinOf(s, dt);
   for (int ii = 0; ii < nSteps; ++ii) {
      /* half kick + drift fused in one kernel (same arithmetic as advanceVelocity(dt/2) then advancePosition(dt)); from the second step
       * on they ride with the previous step's closing half kick (below) */
      if (ii == 0) {
         startTimer(velocityTimer);
         startTimer(positionTimer);
         if (lv.on) advanceVelocityPositionLangevinGpu(&s->gpu, 0.5 * dt, 0.5 * dt, lv.c1, lv.c2, lv.kT, lv.seed, s->stepCount);
         else advanceVelocityPositionGpu(&s->gpu, 0.5 * dt, dt);
         stopTimer(positionTimer);
         stopTimer(velocityTimer);
      }

      /* box deformation: the remap sits behind the drift that has just run (the opening kernel above, or the fused closing kernel of the step before) and in front of
       * the redistribution, on the same stream: the re-binning, the halo images and -- with -a 1 -- the interior force work all see the final geometry */
      if (s->deform && s->stepCount >= (uint64_t)s->deformStart) {
         startTimer(deformTimer);
         deformStep(s, dt);
         stopTimer(deformTimer);
      }

      /* e[] is read by kineticEnergyGpu below only: the last step's forces must carry energies, the others need not
       * (set before redistributeAtoms: with -a 1 it already launches the interior cells' force work) */
      comdSetEnergyNeeded(&s->gpu, ii == nSteps - 1);
      startTimer(redistributeTimer);
      redistributeAtoms(s);
      stopTimer(redistributeTimer);

      startTimer(computeForceTimer);
      computeForce(s);
      stopTimer(computeForceTimer);
      comdSetEnergyNeeded(&s->gpu, 1);
      /* device status words (cell overflow, lost atom, message overflow, row overflow) of the step BEFORE, without a synchronisation: a run with a
       * dropped atom stops a step or two later (round 2: at the next energy read, up to printRate steps on) */
      comdPollStatus(&s->gpu, s->gpu.boundary_stream, "timestep");

      startTimer(velocityTimer);
      if (ii == nSteps - 1) advanceVelocity(s, 0.5 * dt);
      else {
         /* closing half kick of this step + opening half kick and drift of the next: one pass over the atoms, the two kicks still two
          * separate roundings (bit-identical to the three calls of timestep.c:52-58, 95) */
         startTimer(positionTimer);
         if (lv.on) advanceVelocityVelocityPositionLangevinGpu(&s->gpu, 0.5 * dt, 0.5 * dt, 0.5 * dt, lv.c1, lv.c2, lv.kT, lv.seed, s->stepCount + 1);
         else advanceVelocityVelocityPositionGpu(&s->gpu, 0.5 * dt, 0.5 * dt, dt);
         stopTimer(positionTimer);
      }
      stopTimer(velocityTimer);
      s->stepCount++;
   }
   kineticEnergyGpu(s);
   return s->ePotential;
}

void computeForce(SimFlat* s) { s->pot->force(s); }

void kineticEnergyGpu(SimFlat* s)
{
   real_t eLocal[2], eSum[2];
   computeEnergy(&s->gpu, eLocal);
   comdCheckStatus(&s->gpu, "kineticEnergyGpu");      /* cell / message overflow and lost atoms surface here */
   if (s->gpu.do_eam) {
      /* cta_cell, thread_atom: bricks whose block outgrew the LDS image took the thread-per-atom form (correct, many times slower).  The image was sized for the occupancies of
       * the first launch; a system that has changed since (heating, a density front) is noticed here, once per energy read, and the next launch sizes it again */
      int st[3];
      comdEamBrickStats(&s->gpu, st);
      if (st[0] > 0 && (s->method == CTA_CELL || s->method == THREAD_ATOM || s->method == WARP_ATOM)) {
         if (!s->quiet && printRank()) fprintf(stderr, "eamForce: %d brick launches took the thread-per-atom form since the last energy read (image of %d records): re-sizing the image\n", st[0], st[2]);
         comdEamBrickResize(&s->gpu);
      }
   }
   startTimer(commReduceTimer);
   addRealParallel(eLocal, eSum, 2);
   stopTimer(commReduceTimer);
   s->ePotential = eSum[0];
   s->eKinetic = eSum[1];
}

void computePressure(SimFlat* s)
{
   real_t local[12], sum[12];
   computeVirial(&s->gpu, local);
   addRealParallel(local, sum, 12);
   for (int c = 0; c < 6; ++c) { s->W[c] = sum[c]; s->K[c] = sum[6 + c]; }
   s->V = s->domain->globalExtent[0] * s->domain->globalExtent[1] * s->domain->globalExtent[2];
}

int comdPairHistogram(SimFlat* s, int nBins, double rMax, double* outCounts)
{
   const double cutoff = s->pot->cutoff;
   if (rMax <= 0.0) rMax = cutoff;
   if (nBins < 1 || nBins > COMD_RDF_MAX_BINS || !(rMax <= cutoff)) return -1;
   uint64_t* local = (uint64_t*)malloc((size_t)nBins * sizeof(uint64_t));
   double* mine = (double*)malloc((size_t)nBins * sizeof(double));
   computePairHistogram(&s->gpu, nBins, (real_t)rMax, local);
   for (int k = 0; k < nBins; ++k) mine[k] = (double)local[k];
   addDoubleParallel(mine, outCounts, nBins);
   for (int k = 0; k < nBins; ++k) outCounts[k] *= 0.5;
   free(local); free(mine);
   return 0;
}

/* ---- centro-symmetry and coordination (not in the reference; comd_host.h) ---- */
double comdDefaultCoordRadius(SimFlat* s)
{
   const double r = 0.5 * (M_SQRT1_2 + 1.0) * s->lat, cutoff = s->pot->cutoff;
   return r < cutoff ? r : cutoff;
}

int comdCentroSymmetry(SimFlat* s, double rCoord, double* cspByGid, double* coordByGid)
{
   const double cutoff = s->pot->cutoff;
   if (rCoord <= 0.0) rCoord = comdDefaultCoordRadius(s);
   if (!(rCoord <= cutoff)) return -1;
   const int cap = s->boxes->maxAtoms, nLocalBoxes = s->boxes->nLocalBoxes;
   const size_t nSlots = (size_t)nLocalBoxes * cap, n = (size_t)s->atoms->nGlobal;
   /* staging for the by-slot arrays, kept with the simulation: fresh pages for 64 MB at 80^3 would cost more than the kernel */
   const size_t need = (nSlots + 1) * (sizeof(real_t) + 2 * sizeof(int)) + ((size_t)nLocalBoxes + 1) * sizeof(int);
   if (need > s->cspStageBytes) { free(s->cspStage); s->cspStage = malloc(need); s->cspStageBytes = need; }
   real_t* csp = (real_t*)s->cspStage;
   int* coord = (int*)(csp + nSlots + 1);
   int* gid = coord + nSlots + 1;
   int* nAtoms = gid + nSlots + 1;
   computeCentroSymmetry(&s->gpu, (real_t)rCoord, csp, coord);          /* blocks: the stream is drained, the two copies below see the same state */
   comdMemcpyDtoH(gid, s->gpu.atoms.gid, (long)(nSlots * sizeof(int)));
   comdMemcpyDtoH(nAtoms, s->gpu.boxes.nAtoms, (long)((size_t)nLocalBoxes * sizeof(int)));
   const int one = getNRanks() == 1;
   double* mine = one ? NULL : (double*)calloc(n ? 2 * n : 1, sizeof(double));
   double* outCsp = one ? cspByGid : mine;
   double* outCoord = one ? coordByGid : mine + n;
   if (one) { memset(cspByGid, 0, n * sizeof(double)); memset(coordByGid, 0, n * sizeof(double)); }
   for (int b = 0; b < nLocalBoxes; ++b)
      for (size_t o = (size_t)b * cap, e = o + (size_t)nAtoms[b]; o < e; ++o) {
         const size_t g = (size_t)gid[o];
         if (g < n) { outCsp[g] = (double)csp[o]; outCoord[g] = (double)coord[o]; }
      }
   if (!one) {
      /* every other rank holds 0 for a gid (and inf + 0 = inf); in chunks whose count fits addDoubleParallel's int */
      const size_t chunk = (size_t)1 << 28;
      startTimer(commReduceTimer);
      for (size_t o = 0; o < n; o += chunk) {
         const int len = (int)(n - o < chunk ? n - o : chunk);
         addDoubleParallel(mine + o, cspByGid + o, len);
         addDoubleParallel(mine + n + o, coordByGid + o, len);
      }
      stopTimer(commReduceTimer);
   }
   free(mine);
   return 0;
}

/* ---- adaptive common neighbour analysis (not in the reference; comd_host.h) ---- */
int comdCommonNeighbors(SimFlat* s, int* typeByGid, long long counts[5])
{
   const int cap = s->boxes->maxAtoms, nLocalBoxes = s->boxes->nLocalBoxes;
   const size_t nSlots = (size_t)nLocalBoxes * cap, n = (size_t)s->atoms->nGlobal;
   /* staging for the by-slot arrays, kept with the simulation as comdCentroSymmetry's */
   const size_t need = (2 * (nSlots + 1) + (size_t)nLocalBoxes + 1) * sizeof(int);
   if (need > s->cnaStageBytes) { free(s->cnaStage); s->cnaStage = malloc(need); s->cnaStageBytes = need; }
   int* type = (int*)s->cnaStage;
   int* gid = type + nSlots + 1;
   int* nAtoms = gid + nSlots + 1;
   computeCommonNeighbors(&s->gpu, type);          /* blocks: the stream is drained, the two copies below see the same state */
   comdMemcpyDtoH(gid, s->gpu.atoms.gid, (long)(nSlots * sizeof(int)));
   comdMemcpyDtoH(nAtoms, s->gpu.boxes.nAtoms, (long)((size_t)nLocalBoxes * sizeof(int)));
   const int one = getNRanks() == 1;
   int* mine = one ? typeByGid : (int*)malloc((n ? n : 1) * sizeof(int));
   memset(mine, 0, n * sizeof(int));
   for (int b = 0; b < nLocalBoxes; ++b)
      for (size_t o = (size_t)b * cap, e = o + (size_t)nAtoms[b]; o < e; ++o) {
         const size_t g = (size_t)gid[o];
         if (g < n) mine[g] = type[o];
      }
   if (!one) {
      /* every other rank holds 0 for a gid; in chunks whose count fits addIntParallel's int */
      const size_t chunk = (size_t)1 << 28;
      startTimer(commReduceTimer);
      for (size_t o = 0; o < n; o += chunk) addIntParallel(mine + o, typeByGid + o, (int)(n - o < chunk ? n - o : chunk));
      stopTimer(commReduceTimer);
      free(mine);
   }
   for (int t = 0; t < 5; ++t) counts[t] = 0;
   for (size_t g = 0; g < n; ++g) { const int t = typeByGid[g]; counts[t >= 0 && t <= 4 ? t : 0] += 1; }
   return 0;
}

/* ---- per-atom virial stress (not in the reference; comd_host.h) ---- */
int comdAtomStress(SimFlat* s, int withKinetic, double* stressByGid)
{
   if (!s->gpu.boxes.nAtoms) return -1;
   const int cap = s->boxes->maxAtoms, nLocalBoxes = s->boxes->nLocalBoxes;
   const size_t nSlots = (size_t)nLocalBoxes * cap, n = (size_t)s->atoms->nGlobal;
   /* staging for the by-slot planes, kept with the simulation as comdCentroSymmetry's */
   const size_t need = (6 * nSlots + 1) * sizeof(real_t) + (nSlots + 1 + (size_t)nLocalBoxes + 1) * sizeof(int);
   if (need > s->stressStageBytes) { free(s->stressStage); s->stressStage = malloc(need); s->stressStageBytes = need; }
   real_t* planes = (real_t*)s->stressStage;
   int* gid = (int*)(planes + 6 * nSlots + 1);
   int* nAtoms = gid + nSlots + 1;
   computeAtomStress(&s->gpu, withKinetic, planes);          /* blocks: the stream is drained, the two copies below see the same state */
   comdMemcpyDtoH(gid, s->gpu.atoms.gid, (long)(nSlots * sizeof(int)));
   comdMemcpyDtoH(nAtoms, s->gpu.boxes.nAtoms, (long)((size_t)nLocalBoxes * sizeof(int)));
   const int one = getNRanks() == 1;
   double* mine = one ? stressByGid : (double*)malloc((n ? 6 * n : 1) * sizeof(double));
   memset(mine, 0, 6 * n * sizeof(double));
   for (int b = 0; b < nLocalBoxes; ++b)
      for (size_t o = (size_t)b * cap, e = o + (size_t)nAtoms[b]; o < e; ++o) {
         const size_t g = (size_t)gid[o];
         if (g < n) for (int c = 0; c < 6; ++c) mine[6 * g + c] = (double)planes[(size_t)c * nSlots + o];
      }
   if (!one) {
      /* every other rank holds 0 for a gid; in chunks whose count fits addDoubleParallel's int */
      const size_t chunk = (size_t)1 << 28;
      startTimer(commReduceTimer);
      for (size_t o = 0; o < 6 * n; o += chunk) addDoubleParallel(mine + o, stressByGid + o, (int)(6 * n - o < chunk ? 6 * n - o : chunk));
      stopTimer(commReduceTimer);
      free(mine);
   }
   return 0;
}

int comdStressSummary(SimFlat* s, int withKinetic, double* out7)
{
   if (!s->gpu.boxes.nAtoms) return -1;
   const double n = (double)s->atoms->nGlobal;
   const double omega = (double)s->domain->globalExtent[0] * s->domain->globalExtent[1] * s->domain->globalExtent[2] / (n > 0.0 ? n : 1.0);
   double local[7];
   computeAtomStress(&s->gpu, withKinetic, NULL);
   computeAtomStressSummary(&s->gpu, omega, local);
   const int nRanks = getNRanks(), me = getMyRank();
   if (nRanks > 1) {
      /* the sums add; the extremes and the gid go through one slot per rank of a summed vector (no MIN/MAX of doubles in the transport), taken in rank order */
      double* mine = (double*)calloc(2 * (size_t)(3 + 4 * nRanks), sizeof(double));
      double* all = mine + 3 + 4 * (size_t)nRanks;
      mine[0] = local[0]; mine[1] = local[3]; mine[2] = local[6];
      if (local[6] > 0.0) { double* slot = mine + 3 + 4 * (size_t)me; slot[0] = local[1]; slot[1] = local[2]; slot[2] = local[4]; slot[3] = local[5] + 1.0; }
      startTimer(commReduceTimer);
      addDoubleParallel(mine, all, 3 + 4 * nRanks);
      stopTimer(commReduceTimer);
      local[0] = all[0]; local[3] = all[1]; local[6] = all[2];
      local[1] = INFINITY; local[2] = -INFINITY; local[4] = -INFINITY; local[5] = -1.0;
      for (int r = 0; r < nRanks; ++r) {
         const double* slot = all + 3 + 4 * (size_t)r;
         if (slot[3] == 0.0) continue;          /* a rank without atoms */
         const double g = slot[3] - 1.0;
         if (slot[0] < local[1]) local[1] = slot[0];
         if (slot[1] > local[2]) local[2] = slot[1];
         if (local[5] < 0.0 || slot[2] > local[4] || (slot[2] == local[4] && g < local[5])) { local[4] = slot[2]; local[5] = g; }
      }
      free(mine);
   }
   const double N = local[6];
   out7[0] = N > 0.0 ? local[0] / N : 0.0; out7[1] = local[1]; out7[2] = local[2];
   out7[3] = N > 0.0 ? local[3] / N : 0.0; out7[4] = local[4]; out7[5] = local[5]; out7[6] = N;
   return 0;
}

/* ---- per-atom strain and D^2min (not in the reference; comd_host.h) ---- */
int comdStrainReference(SimFlat* s, int on)
{
   if (!s->gpu.boxes.nAtoms) return -1;
   const int nGlobal = s->atoms->nGlobal;
   int fail = comdStrainReferenceGpu(&s->gpu, nGlobal, on), anyFail = 0;
   maxIntParallel(&fail, &anyFail, 1);
   if (anyFail && !fail) comdStrainReferenceGpu(&s->gpu, nGlobal, 0);      /* all ranks or none */
   s->strainHasRef = on != 0 && !anyFail;
   if (!s->strainHasRef) return anyFail;
   for (int a = 0; a < 3; ++a) s->strainL0[a] = s->gpu.strainL0[a] = (double)s->domain->globalExtent[a];
   if (getNRanks() > 1) {
      /* halo neighbours need the records of the other ranks' atoms: every other rank holds 0 for a gid; in chunks whose count fits addDoubleParallel's int */
      const size_t n = 4 * (size_t)nGlobal, chunk = (size_t)1 << 28;
      double* mine = (double*)malloc(2 * n * sizeof(double));
      double* all = mine + n;
      comdMemcpyDtoH(mine, s->gpu.strainRefBuf, (long)(n * sizeof(double)));
      startTimer(commReduceTimer);
      for (size_t o = 0; o < n; o += chunk) addDoubleParallel(mine + o, all + o, (int)(n - o < chunk ? n - o : chunk));
      stopTimer(commReduceTimer);
      comdMemcpyHtoD(s->gpu.strainRefBuf, all, (long)(n * sizeof(double)));
      free(mine);
   }
   return 0;
}

int comdStrainReferenceBox(SimFlat* s, double* L0)
{
   if (!s->strainHasRef) return -1;
   for (int a = 0; a < 3; ++a) L0[a] = s->strainL0[a];
   return 0;
}

/* the radius the two entries launch with: the default for rCut <= 0; 0 when the entry has to refuse */
static double strainRadius(SimFlat* s, double rCut)
{
   if (!s->gpu.boxes.nAtoms || !s->strainHasRef) return 0.0;
   if (rCut <= 0.0) rCut = comdDefaultCoordRadius(s);
   return rCut <= s->pot->cutoff ? rCut : 0.0;
}

int comdAtomStrain(SimFlat* s, double rCut, double* strainByGid7, int* countByGid)
{
   rCut = strainRadius(s, rCut);
   if (!(rCut > 0.0)) return -1;
   const int cap = s->boxes->maxAtoms, nLocalBoxes = s->boxes->nLocalBoxes;
   const size_t nSlots = (size_t)nLocalBoxes * cap, n = (size_t)s->atoms->nGlobal;
   /* staging for the by-slot planes, kept with the simulation as comdCentroSymmetry's */
   const size_t need = (7 * nSlots + 1) * sizeof(real_t) + (2 * (nSlots + 1) + (size_t)nLocalBoxes + 1) * sizeof(int);
   if (need > s->strainStageBytes) { free(s->strainStage); s->strainStage = malloc(need); s->strainStageBytes = need; }
   real_t* planes = (real_t*)s->strainStage;
   int* count = (int*)(planes + 7 * nSlots + 1);
   int* gid = count + nSlots + 1;
   int* nAtoms = gid + nSlots + 1;
   computeAtomStrain(&s->gpu, (real_t)rCut, planes, count);          /* blocks: the stream is drained, the two copies below see the same state */
   comdMemcpyDtoH(gid, s->gpu.atoms.gid, (long)(nSlots * sizeof(int)));
   comdMemcpyDtoH(nAtoms, s->gpu.boxes.nAtoms, (long)((size_t)nLocalBoxes * sizeof(int)));
   const int one = getNRanks() == 1;
   double* mine = one ? strainByGid7 : (double*)malloc((n ? 7 * n : 1) * sizeof(double));
   int* mineN = one ? countByGid : (int*)malloc((n ? n : 1) * sizeof(int));
   memset(mine, 0, 7 * n * sizeof(double));
   memset(mineN, 0, n * sizeof(int));
   for (int b = 0; b < nLocalBoxes; ++b)
      for (size_t o = (size_t)b * cap, e = o + (size_t)nAtoms[b]; o < e; ++o) {
         const size_t g = (size_t)gid[o];
         if (g < n) { for (int c = 0; c < 7; ++c) mine[7 * g + c] = (double)planes[(size_t)c * nSlots + o]; mineN[g] = count[o]; }
      }
   if (!one) {
      /* every other rank holds 0 for a gid (and NaN + 0 = NaN, an invalid atom stays one); in chunks whose count fits the int of the sums */
      const size_t chunk = (size_t)1 << 28;
      startTimer(commReduceTimer);
      for (size_t o = 0; o < 7 * n; o += chunk) addDoubleParallel(mine + o, strainByGid7 + o, (int)(7 * n - o < chunk ? 7 * n - o : chunk));
      for (size_t o = 0; o < n; o += chunk) addIntParallel(mineN + o, countByGid + o, (int)(n - o < chunk ? n - o : chunk));
      stopTimer(commReduceTimer);
      free(mine); free(mineN);
   }
   return 0;
}

int comdStrainSummary(SimFlat* s, double rCut, double threshold, double* out9)
{
   rCut = strainRadius(s, rCut);
   if (!(rCut > 0.0) || !(threshold > 0.0)) return -1;
   double local[9];          /* sum gamma, max gamma, gid, sum vol, sum D^2, max D^2, valid, invalid, above (computeAtomStrainSummary) */
   computeAtomStrain(&s->gpu, (real_t)rCut, NULL, NULL);
   computeAtomStrainSummary(&s->gpu, threshold, local);
   const int nRanks = getNRanks(), me = getMyRank();
   if (nRanks > 1) {
      /* the sums add; the extremes and the gid go through one slot per rank of a summed vector (no MAX of doubles in the transport), taken in rank order */
      double* mine = (double*)calloc(2 * (size_t)(6 + 3 * nRanks), sizeof(double));
      double* all = mine + 6 + 3 * (size_t)nRanks;
      mine[0] = local[0]; mine[1] = local[3]; mine[2] = local[4]; mine[3] = local[6]; mine[4] = local[7]; mine[5] = local[8];
      if (local[6] > 0.0) { double* slot = mine + 6 + 3 * (size_t)me; slot[0] = local[1]; slot[1] = local[2] + 1.0; slot[2] = local[5]; }
      startTimer(commReduceTimer);
      addDoubleParallel(mine, all, 6 + 3 * nRanks);
      stopTimer(commReduceTimer);
      local[0] = all[0]; local[3] = all[1]; local[4] = all[2]; local[6] = all[3]; local[7] = all[4]; local[8] = all[5];
      local[1] = -INFINITY; local[2] = -1.0; local[5] = -INFINITY;
      for (int r = 0; r < nRanks; ++r) {
         const double* slot = all + 6 + 3 * (size_t)r;
         if (slot[1] == 0.0) continue;          /* a rank without valid atoms */
         const double g = slot[1] - 1.0;
         if (local[2] < 0.0 || slot[0] > local[1] || (slot[0] == local[1] && g < local[2])) { local[1] = slot[0]; local[2] = g; }
         if (slot[2] > local[5]) local[5] = slot[2];
      }
      free(mine);
   }
   const double N = local[6];
   out9[0] = N + local[7]; out9[1] = local[7];
   out9[2] = N > 0.0 ? local[0] / N : 0.0; out9[3] = N > 0.0 ? local[1] : 0.0; out9[4] = local[2];
   out9[5] = N > 0.0 ? local[3] / N : 0.0; out9[6] = N > 0.0 ? local[4] / N : 0.0; out9[7] = N > 0.0 ? local[5] : 0.0; out9[8] = local[8];
   return 0;
}

/* ---- displacement tracking (not in the reference; comd_host.h) ---- */
int comdTrackDisplacement(SimFlat* s, int on)
{
   int fail = comdTrackDisplacementGpu(&s->gpu, s->atoms->nGlobal, on), anyFail = 0;
   maxIntParallel(&fail, &anyFail, 1);
   if (anyFail && !fail) comdTrackDisplacementGpu(&s->gpu, s->atoms->nGlobal, 0);      /* all ranks or none */
   s->trackDisp = on != 0 && !anyFail;
   return anyFail;
}

#define COMD_DISP_UNIT (1.0 / 4294967296.0)      /* Angstroms per unit of the device records */

int comdDisplacements(SimFlat* s, double* out)
{
   if (!s->trackDisp) return -1;
   const size_t n = (size_t)s->atoms->nGlobal;
   int64_t* raw = (int64_t*)malloc(4 * n * sizeof(int64_t));
   comdCopyDisplacementsGpu(&s->gpu, raw);
   if (getNRanks() == 1) {
      for (size_t g = 0; g < n; ++g) for (int c = 0; c < 3; ++c) out[3 * g + c] = (double)raw[4 * g + c] * COMD_DISP_UNIT;
      free(raw);
      return 0;
   }
   /* the ranks' parts as doubles (exact below 2^53), summed in chunks whose count fits addDoubleParallel's int */
   const int64_t top = (int64_t)1 << 53;
   double* mine = (double*)malloc(3 * n * sizeof(double));
   int bad = 0, anyBad = 0;
   for (size_t g = 0; g < n; ++g)
      for (int c = 0; c < 3; ++c) {
         const int64_t v = raw[4 * g + c];
         if (v >= top || v <= -top) bad = 1;
         mine[3 * g + c] = (double)v;
      }
   free(raw);
   maxIntParallel(&bad, &anyBad, 1);
   if (!anyBad) {
      const size_t chunk = (size_t)1 << 28;
      startTimer(commReduceTimer);
      for (size_t o = 0; o < 3 * n; o += chunk) addDoubleParallel(mine + o, out + o, (int)(3 * n - o < chunk ? 3 * n - o : chunk));
      stopTimer(commReduceTimer);
      for (size_t k = 0; k < 3 * n; ++k) out[k] *= COMD_DISP_UNIT;
   }
   free(mine);
   return anyBad ? -2 : 0;
}

int comdMsd(SimFlat* s, double* out7)
{
   if (!s->trackDisp) return -1;
   const size_t n = (size_t)s->atoms->nGlobal;
   out7[6] = (double)n;
   if (getNRanks() == 1) { computeDisplacementSums(&s->gpu, out7); return 0; }
   double* d = (double*)malloc(3 * n * sizeof(double));
   const int rc = comdDisplacements(s, d);
   for (int c = 0; c < 6; ++c) out7[c] = 0.0;
   if (rc == 0)
      for (size_t g = 0; g < n; ++g)
         for (int c = 0; c < 3; ++c) { const double v = d[3 * g + c]; out7[c] += v; out7[3 + c] += v * v; }
   free(d);
   return rc;
}

double pressureOf(const SimFlat* s)
{
   return ((double)s->K[0] + s->K[1] + s->K[2] + s->W[0] + s->W[1] + s->W[2]) / (3.0 * s->V);
}

static void launchInteriorForce(SimFlat* sim)
{
   SimGpu* g = &sim->gpu;
   if (sim->gpu.do_eam) {
      eamForce1GpuAsync(g, g->n_interior_cells, g->interior_cells, sim->method, g->interior_stream, sim->spline);
      eamForce2GpuAsync(g, g->n_interior_cells, g->interior_cells, sim->method, g->interior_stream, sim->spline);
   } else {
      ljForceGpuAsync(g, g->n_interior_cells, g->interior_cells, sim->method, g->interior_stream);
   }
   sim->interiorLaunched = 1;
}

/* -a 1: the potentials call this before their boundary work; starts the interior cells if redistributeAtoms could not
 * (a Verlet-list build had to come first) */
void ensureInteriorForceLaunched(SimFlat* sim)
{
   if (sim->gpuAsync && !sim->interiorLaunched) {
      comdStreamSynchronize(sim->gpu.boundary_stream);
      launchInteriorForce(sim);
   }
}

static void redistributeAtomsCells(SimFlat* sim, int overlapInterior);

/* timestep.c:278-352 redistributeAtomsGpuNL.  Lists valid (no atom has moved more than skin/2 since the build, on any rank):
 * nothing is re-binned, atoms keep their slots, only the halo copies' positions are refreshed.  Otherwise: the ordinary
 * redistribution (re-bin, migrate, full atom exchange, gid sort) followed by a list build.  The reference also rebuilds on every
 * rank whenever an atom changed owner (:331-350); here owners only change inside the ordinary redistribution. */
static void redistributeAtomsNL(SimFlat* sim)
{
   SimGpu* g = &sim->gpu;
   /* The reference's rule (gpu_kernels.cu:1449-1484): has an atom moved more than skin/2 since the build?  Asked of the drift kernel that has just run -- a stream
    * synchronisation per step (35 us of device idle at EAM 80^3).  COMD_NL_DEFERRED=1: the form that never drains the stream (comd_hip.h
    * comdNeighborListUpdateDeferredGpu: decided two drifts late against a threshold lowered by what two steps can add) -- measured at -1 % of the step, because the
    * lower threshold rebuilds the lists every 18 instead of every 22 steps; the blocking form stays the default. */
   static int deferred = -1;
   if (deferred < 0) { const char* e = getenv("COMD_NL_DEFERRED"); deferred = e && atoi(e) != 0; }
   /* a box that changes every step changes the thresholds every step: the blocking form */
   int need = deferred && !sim->deform ? comdNeighborListUpdateDeferredGpu(g) : neighborListUpdateRequiredGpu(g), needAll = 0;
   startTimer(commReduceTimer);
   maxIntParallel(&need, &needAll, 1);
   stopTimer(commReduceTimer);
   sim->interiorLaunched = 0;
   if (needAll) {
      /* many steps since the last full exchange: the message counts may have drifted past the agreed slack -- swap exact sizes once */
      invalidateHaloSizes(sim->atomExchange);
      if (sim->gpu.do_eam) invalidateHaloSizes(((EamPotential*)sim->pot)->forceExchange);
      redistributeAtomsCells(sim, 0);
      startTimer(neighborListBuildTimer);
      buildNeighborListGpu(g, sim->method, 0);
      preparePositionExchange(sim->positionExchange, sim);
      stopTimer(neighborListBuildTimer);
      sim->nlBuilds++;
      if (sim->boxChanged) {          /* Lambda = 1 again */
         for (int a = 0; a < 3; ++a) sim->listExtent[a] = (double)sim->domain->globalExtent[a];
         deformListBudget(sim);
      }
   } else {
      if (sim->gpuAsync) { comdStreamSynchronize(g->boundary_stream); launchInteriorForce(sim); }
      startTimer(atomHaloTimer);
      haloExchange(sim->positionExchange, sim);
      stopTimer(atomHaloTimer);
   }
}

void redistributeAtoms(SimFlat* sim)
{
   if (sim->useNL) redistributeAtomsNL(sim);
   else { sim->interiorLaunched = 0; redistributeAtomsCells(sim, 1); }
}

/* timestep.c:222-276 redistributeAtomsGpu */
static void redistributeAtomsCells(SimFlat* sim, int overlapInterior)
{
   SimGpu* g = &sim->gpu;
   /* empties the halo cells, moves atoms that left their cell, compacts + gid-sorts the cells that changed -- the last only when something reads the cells before
    * sortAtomsGpu does it again: a pack kernel (an axis with a real peer) or the interior force launch of the overlap mode */
   g->skipSortAfterUpdate = haloMirrorFirstAxis(sim->atomExchange) == 0 && !(sim->gpuAsync && overlapInterior);
   updateLinkCellsGpu(g, g->boundary_stream);

   if (sim->gpuAsync && overlapInterior) {
      /* local cells are final: start the interior force work while the halo exchange runs (timestep.c:257-265) */
      comdStreamSynchronize(g->boundary_stream);
      launchInteriorForce(sim);
   }

   startTimer(atomHaloTimer);
   haloExchange(sim->atomExchange, sim);
   stopTimer(atomHaloTimer);

   buildAtomListGpu(g, g->boundary_stream);
   sortAtomsGpu(g, g->boundary_stream);          /* halo cells and cells that received migrants */
}
