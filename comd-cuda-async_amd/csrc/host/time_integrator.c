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

/* One step's box: the strained axes are set from box0 and the strained time, never by multiplying up, so they are a pure function of the steps taken; the barostat's
 * axes take what the last coupling asked for; the kernel gets L_new / L_old.  With the barostat on, an axis without a rate keeps its extent (or takes the barostat's);
 * without it every axis goes through extentsAt, as before the barostat existed.  A box the grid cannot follow ends the run here, before anything is launched. */
static void deformStep(SimFlat* s, real_t dt, int strain)
{
   double L[3], E[3];
   for (int a = 0; a < 3; ++a) L[a] = (double)s->domain->globalExtent[a];
   if (strain) {
      s->deformTime += (double)dt;
      extentsAt(s, s->deformTime, E);
      for (int a = 0; a < 3; ++a) if (!s->baro || s->erate[a] != 0.0) L[a] = E[a];
   }
   if (s->baroPending) {
      for (int a = 0; a < 3; ++a) if (s->baroAxes >> a & 1) L[a] = s->baroNext[a];
      s->baroPending = 0;
   }
   if (comdSetBox(s, L) != 0) {
      if (printRank())
         printf("Error: at step %llu the box [ %g, %g, %g ] would make a link cell narrower than the %g Angstroms the grid was built for (or is not positive); "
                "re-gridding is not implemented.\n", (unsigned long long)s->stepCount, L[0], L[1], L[2], (double)s->boxes->builtRange);
      fflush(stdout);
      exit(-1);
   }
   if (strain) {
      extentsAt(s, s->deformTime + (double)dt, E);
      for (int a = 0; a < 3; ++a) if (!s->baro || s->erate[a] != 0.0) s->nextExtent[a] = E[a];
   }
   deformListBudget(s);
}

/* ---- Berendsen barostat (not in the reference; comd_host.h) ---- */
/* the cube root of x > 0 to well within an ulp: the library's (which may be 2 ulp off) and one Newton step whose residual y^3 - x is formed with the exact error of y * y */
static double cbrtRefined(double x)
{
   const double y = cbrt(x), y2 = y * y, e2 = fma(y, y, -y2);
   const double residual = fma(y2, y, -x) + e2 * y;
   return y - residual / (3.0 * y2);
}

int comdBerendsenScale(const double p[3], const double target[3], double dtCoupling, double tau, double modulus, int axesMask, int iso, double mu[3])
{
   for (int a = 0; a < 3; ++a) if (!isfinite(p[a]) || !isfinite(target[a])) return -1;
   if (!isfinite(dtCoupling) || !isfinite(tau) || !isfinite(modulus)) return -1;
   if (!(tau > 0.0) || !(modulus > 0.0) || dtCoupling > tau || dtCoupling < 0.0 || axesMask < 1 || axesMask > 7) return -1;
   double m[3] = { 1.0, 1.0, 1.0 };
   if (iso) {
      double pm = 0.0, tm = 0.0; int n = 0;
      for (int a = 0; a < 3; ++a) if (axesMask >> a & 1) { pm += p[a]; tm += target[a]; n++; }
      pm /= n; tm /= n;
      const double x = 1.0 - (dtCoupling / tau) * (tm - pm) / modulus;
      if (!(x > 0.0)) return -1;
      for (int a = 0; a < 3; ++a) if (axesMask >> a & 1) m[a] = cbrtRefined(x);
   } else {
      for (int a = 0; a < 3; ++a) if (axesMask >> a & 1) {
         const double x = 1.0 - (dtCoupling / tau) * (target[a] - p[a]) / modulus;
         if (!(x > 0.0)) return -1;
         m[a] = cbrtRefined(x);
      }
   }
   for (int a = 0; a < 3; ++a) mu[a] = m[a];
   return 0;
}

/* why a setting is refused: 0 fine, 1 profile mode, 2 an axis that also strains, 3 every, 4 the mask, 5 the scale rule's own refusals */
int comdBarostatRefusal(const SimFlat* s, const double targetGPa[3], double tauFs, double modulusGPa, int every, int axesMask)
{
   double mu[3];
   if (s->gpuProfile) return 1;
   if (axesMask < 1 || axesMask > 7) return 4;
   for (int a = 0; a < 3; ++a) if ((axesMask >> a & 1) && s->erate[a] != 0.0) return 2;
   if (every < 1) return 3;
   if (comdBerendsenScale(targetGPa, targetGPa, (double)every * s->dt, tauFs, modulusGPa, axesMask, 0, mu) != 0) return 5;
   return 0;
}

int comdSetBarostat(SimFlat* s, int on, const double targetGPa[3], double tauFs, double modulusGPa, int every, int axesMask, int iso)
{
   if (!on) {
      /* a coupling whose box has not been set yet is dropped with the barostat */
      if (s->baroPending) for (int a = 0; a < 3; ++a) if (s->baroAxes >> a & 1) s->nextExtent[a] = (double)s->domain->globalExtent[a];
      s->baro = 0; s->baroPending = 0;
      return 0;
   }
   if (!s->gpu.boxes.nAtoms || comdBarostatRefusal(s, targetGPa, tauFs, modulusGPa, every, axesMask) != 0) return -1;
   for (int a = 0; a < 3; ++a) s->baroTarget[a] = targetGPa[a];
   s->baroTau = tauFs; s->baroModulus = modulusGPa; s->baroEvery = every; s->baroAxes = axesMask; s->baroIso = iso != 0;
   s->baroPending = 0;
   s->baro = 1;
   return 0;
}

int comdGetBarostat(SimFlat* s, double out8[8])
{
   for (int a = 0; a < 3; ++a) out8[a] = s->baroTarget[a];
   out8[3] = s->baroTau; out8[4] = s->baroModulus; out8[5] = (double)s->baroEvery; out8[6] = (double)s->baroAxes; out8[7] = (double)s->baroIso;
   return s->baro;
}

/* the step that has just closed (its forces and its closing half kick are done) couples: p from the fast evaluation, mu, and the box the remap of the coming step
 * will set.  The list rule learns the coming extents here, a step ahead, as it does for strain rates. */
static void baroCouple(SimFlat* s, real_t dt)
{
   double wk[13], p[3], mu[3];
   comdVirialFdotr(s, wk);
   for (int a = 0; a < 3; ++a) p[a] = (wk[6 + a] + wk[a]) / wk[12] * eVperA3inGPa;
   if (comdBerendsenScale(p, s->baroTarget, (double)s->baroEvery * (double)dt, s->baroTau, s->baroModulus, s->baroAxes, s->baroIso, mu) != 0) {
      if (printRank())
         printf("Error: at step %llu the barostat cannot scale the box: pressure [ %g, %g, %g ] GPa, coupling interval %g fs against --baroTau %g fs.\n",
                (unsigned long long)s->stepCount + 1, p[0], p[1], p[2], (double)s->baroEvery * (double)dt, s->baroTau);
      fflush(stdout);
      exit(-1);
   }
   for (int a = 0; a < 3; ++a) {
      s->baroNext[a] = (double)s->domain->globalExtent[a] * mu[a];
      if (s->baroAxes >> a & 1) s->nextExtent[a] = s->baroNext[a];
   }
   s->baroPending = 1;
   deformListBudget(s);
   if (s->baroReport) {
      double* row = (double*)nextRow(&s->baroRows, 12 * sizeof(double));
      row[0] = (double)(s->stepCount + 1); row[1] = row[0] * (double)dt;
      for (int a = 0; a < 3; ++a) { row[2 + a] = p[a]; row[5 + a] = mu[a]; row[8 + a] = s->baroAxes >> a & 1 ? s->baroNext[a] : (double)s->domain->globalExtent[a]; }
      row[11] = row[8] * row[9] * row[10];
   }
}

/* ---- Mueller-Plathe exchange (not in the reference; comd_host.h) ---- */
int comdSetMullerPlathe(SimFlat* s, int on, int axis, int nBins, int every, int swaps, int start)
{
   if (!on) { s->mp = 0; return 0; }
   if (!s->gpu.boxes.nAtoms || start < 0 || comdMullerPlatheRefusal(axis, nBins, every, swaps) != 0) return -1;
   s->mpAxis = axis; s->mpBins = nBins; s->mpEvery = every; s->mpSwaps = swaps; s->mpStart = start;
   s->mp = 1;
   return 0;
}

int comdGetMullerPlathe(SimFlat* s, double out8[8])
{
   out8[0] = (double)s->mpAxis; out8[1] = (double)s->mpBins; out8[2] = (double)s->mpEvery; out8[3] = (double)s->mpSwaps; out8[4] = (double)s->mpStart;
   out8[5] = s->mpExchanged; out8[6] = (double)s->mpPairs; out8[7] = (double)s->mpSkipped;
   return s->mp;
}

/* the step that has just closed exchanges: positions and forces stay, so nothing is redistributed or evaluated again; the next step opens with the new momenta */
static void mpExchange(SimFlat* s, real_t dt)
{
   int pairs[2 * COMD_MP_MAX_SWAPS], skipped = 0;
   double dE = 0.0;
   const int kept = comdMullerPlatheSwap(s, s->mpAxis, s->mpBins, s->mpSwaps, pairs, &dE, &skipped);
   /* --mp: the energy of the exchanges up to global step profStart is not part of the flux the profile answers */
   if (s->profile && s->stepCount + 1 <= (uint64_t)s->profStart) s->mpExchangedAtProfStart = s->mpExchanged;
   if (s->mpReport) {
      double* row = (double*)nextRow(&s->mpRows, 6 * sizeof(double));
      row[0] = (double)(s->stepCount + 1); row[1] = row[0] * (double)dt; row[2] = (double)kept; row[3] = (double)skipped; row[4] = dE; row[5] = s->mpExchanged;
   }
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
   if (s->baro) for (int a = 0; a < 3; ++a) if (r[a] != 0.0 && (s->baroAxes >> a & 1)) return -1;      /* an axis is strained or pressure-coupled, not both */
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
   int split = 1;      /* the step before did not carry this step's opening kick and drift: the first step of a call, and the step behind a coupling */
   for (int ii = 0; ii < nSteps; ++ii) {
      /* half kick + drift fused in one kernel (same arithmetic as advanceVelocity(dt/2) then advancePosition(dt)); from the second step
       * on they ride with the previous step's closing half kick (below) */
      if (split) {
         startTimer(velocityTimer);
         startTimer(positionTimer);
         if (lv.on) advanceVelocityPositionLangevinGpu(&s->gpu, 0.5 * dt, 0.5 * dt, lv.c1, lv.c2, lv.kT, lv.seed, s->stepCount);
         else advanceVelocityPositionGpu(&s->gpu, 0.5 * dt, dt);
         stopTimer(positionTimer);
         stopTimer(velocityTimer);
      }

      /* box deformation: the remap sits behind the drift that has just run (the opening kernel above, or the fused closing kernel of the step before) and in front of
       * the redistribution, on the same stream: the re-binning, the halo images and -- with -a 1 -- the interior force work all see the final geometry */
      const int strain = s->deform && s->stepCount >= (uint64_t)s->deformStart;
      if (strain || s->baroPending) {
         startTimer(deformTimer);
         deformStep(s, dt, strain);
         stopTimer(deformTimer);
      }
      /* barostat: a coupling step ends unfused, the way the last step of a call does (the same roundings), so that the pressure is read between its closing half kick
       * and the next step's opening one; couplings are counted by the global step, so step(4); step(6) couples where step(10) does */
      const int couple = s->baro && s->stepCount + 1 > (uint64_t)s->baroStart && (s->stepCount + 1 - (uint64_t)s->baroStart) % (uint64_t)s->baroEvery == 0;
      /* Mueller-Plathe exchange: the same, behind the closing half kick and in front of the coupling; counted by the global step as well */
      const int swap = s->mp && s->stepCount + 1 > (uint64_t)s->mpStart && (s->stepCount + 1 - (uint64_t)s->mpStart) % (uint64_t)s->mpEvery == 0;
      split = ii == nSteps - 1 || couple || swap;

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
      if (split) advanceVelocity(s, 0.5 * dt);
      else {
         /* closing half kick of this step + opening half kick and drift of the next: one pass over the atoms, the two kicks still two
          * separate roundings (bit-identical to the three calls of timestep.c:52-58, 95) */
         startTimer(positionTimer);
         if (lv.on) advanceVelocityVelocityPositionLangevinGpu(&s->gpu, 0.5 * dt, 0.5 * dt, 0.5 * dt, lv.c1, lv.c2, lv.kT, lv.seed, s->stepCount + 1);
         else advanceVelocityVelocityPositionGpu(&s->gpu, 0.5 * dt, 0.5 * dt, dt);
         stopTimer(positionTimer);
      }
      stopTimer(velocityTimer);
      if (swap) {
         startTimer(mpTimer);
         mpExchange(s, dt);
         stopTimer(mpTimer);
      }
      if (couple) {
         startTimer(baroTimer);
         baroCouple(s, dt);
         stopTimer(baroTimer);
      }
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
   int need = deferred && !sim->deform && !sim->baro ? comdNeighborListUpdateDeferredGpu(g) : neighborListUpdateRequiredGpu(g), needAll = 0;
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
