/* analysis.c -- the host entries of the analyses (not in the reference; comd_host.h): pressure, g(r), centro-symmetry, common neighbour analysis, per-atom
 * stress and strain, Steinhardt order, the Born matrix and the elastic constants, heat flux and its autocorrelation, displacements, slab profiles, the Mueller-Plathe exchange and the structure factor.  Each is a call into include/comd_hip.h for this rank's share and a sum over the ranks. */
#include "comd_host.h"
#include "slot_gather.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

void computePressure(SimFlat* s)
{
   real_t local[12], sum[12];
   computeVirial(&s->gpu, local);
   addRealParallel(local, sum, 12);
   for (int c = 0; c < 6; ++c) { s->W[c] = sum[c]; s->K[c] = sum[6 + c]; }
   s->V = s->domain->globalExtent[0] * s->domain->globalExtent[1] * s->domain->globalExtent[2];
}

/* the fast pressure (comd_host.h): this rank's share from computeVirialFdotr on the box of now, summed over the ranks.  The work list is built and uploaded once */
void comdVirialFdotr(SimFlat* s, double out[13])
{
   if (!s->facePairs) {
      s->nFacePairs = comdPeriodicFacePairs(s, NULL, 0);
      s->facePairs = (int*)malloc(5 * (size_t)(s->nFacePairs > 0 ? s->nFacePairs : 1) * sizeof(int));
      comdPeriodicFacePairs(s, s->facePairs, s->nFacePairs);
      comdSetFacePairsGpu(&s->gpu, s->facePairs, s->nFacePairs);
   }
   double box[3];
   real_t local[12], sum[12];
   for (int a = 0; a < 3; ++a) box[a] = (double)s->domain->globalExtent[a];
   computeVirialFdotr(&s->gpu, box, local);
   startTimer(commReduceTimer);
   addRealParallel(local, sum, 12);
   stopTimer(commReduceTimer);
   for (int c = 0; c < 12; ++c) out[c] = (double)sum[c];
   out[12] = box[0] * box[1] * box[2];
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

/* ---- the by-gid gather of comdCentroSymmetry, comdCommonNeighbors, comdAtomStress, comdAtomStrain, comdSteinhardt and comdAtomHeatFlux ----
 * An output is out[nGlobal][width], filled from `width` consecutive by-slot planes of one kind (slot_gather.h); the real_t outputs come first.  `run` launches the
 * kernel and copies its planes into plane[k], one pointer per output. */
typedef struct { void* out; int kind, width; } GidOutput;
typedef void (*SlotKernel)(SimFlat* s, void* const* plane, const void* arg);

static void gatherByGid(SimFlat* s, SlotKernel run, const void* arg, const GidOutput* out, int nOut)
{
   const int cap = s->boxes->maxAtoms, nLocalBoxes = s->boxes->nLocalBoxes;
   const size_t nSlots = (size_t)nLocalBoxes * cap, n = (size_t)s->atoms->nGlobal;
   /* staging for the by-slot arrays, kept with the simulation: fresh pages for 64 MB at 80^3 would cost more than the kernel */
   size_t need = (nSlots + 1 + (size_t)nLocalBoxes + 1) * sizeof(int), bytes[2];
   for (int k = 0; k < nOut; ++k) need += bytes[k] = ((size_t)out[k].width * nSlots + 1) * (out[k].kind == SLOT_REAL ? sizeof(real_t) : sizeof(int));
   if (need > s->analysisStageBytes) { free(s->analysisStage); s->analysisStage = malloc(need); s->analysisStageBytes = need; }
   char* at = (char*)s->analysisStage;
   void* plane[2];
   for (int k = 0; k < nOut; ++k) { plane[k] = at; at += bytes[k]; }
   int* gid = (int*)at;
   int* nAtoms = gid + nSlots + 1;
   run(s, plane, arg);          /* blocks: the stream is drained, the two copies below see the same state */
   comdMemcpyDtoH(gid, s->gpu.atoms.gid, (long)(nSlots * sizeof(int)));
   comdMemcpyDtoH(nAtoms, s->gpu.boxes.nAtoms, (long)((size_t)nLocalBoxes * sizeof(int)));
   /* one rank writes straight into the caller's arrays */
   const int one = getNRanks() == 1;
   void* mine[2];
   SlotPlane planes[10];
   int nPlanes = 0;
   for (int k = 0; k < nOut; ++k) {
      const size_t len = (size_t)out[k].width * n;
      mine[k] = one ? out[k].out : malloc((len ? len : 1) * (out[k].kind == SLOT_INT ? sizeof(int) : sizeof(double)));
      for (int c = 0; c < out[k].width; ++c) {
         const size_t from = (size_t)c * nSlots * (out[k].kind == SLOT_REAL ? sizeof(real_t) : sizeof(int));
         planes[nPlanes++] = (SlotPlane){ (const char*)plane[k] + from, out[k].kind, mine[k], (size_t)out[k].width, (size_t)c };
      }
   }
   slotGather(nAtoms, gid, nLocalBoxes, cap, n, planes, nPlanes);
   if (one) return;
   /* every other rank holds 0 for a gid (and inf + 0 = inf, NaN + 0 = NaN: an atom without a value stays one) */
   startTimer(commReduceTimer);
   for (int k = 0; k < nOut; ++k) {
      if (out[k].kind == SLOT_INT) addIntParallelLong((int*)mine[k], (int*)out[k].out, (size_t)out[k].width * n);
      else addDoubleParallelLong((double*)mine[k], (double*)out[k].out, (size_t)out[k].width * n);
   }
   stopTimer(commReduceTimer);
   for (int k = 0; k < nOut; ++k) free(mine[k]);
}

static void runCentroSymmetry(SimFlat* s, void* const* plane, const void* rCoord)
{
   computeCentroSymmetry(&s->gpu, *(const real_t*)rCoord, (real_t*)plane[0], (int*)plane[1]);
}

int comdCentroSymmetry(SimFlat* s, double rCoord, double* cspByGid, double* coordByGid)
{
   if (rCoord <= 0.0) rCoord = comdDefaultCoordRadius(s);
   if (!(rCoord <= s->pot->cutoff)) return -1;
   const real_t r = (real_t)rCoord;
   const GidOutput out[2] = { { cspByGid, SLOT_REAL, 1 }, { coordByGid, SLOT_INT_AS_DOUBLE, 1 } };
   gatherByGid(s, runCentroSymmetry, &r, out, 2);
   return 0;
}

/* ---- adaptive common neighbour analysis (not in the reference; comd_host.h) ---- */
static void runCommonNeighbors(SimFlat* s, void* const* plane, const void* none) { computeCommonNeighbors(&s->gpu, (int*)plane[0]); }

int comdCommonNeighbors(SimFlat* s, int* typeByGid, long long counts[5])
{
   const size_t n = (size_t)s->atoms->nGlobal;
   const GidOutput out = { typeByGid, SLOT_INT, 1 };
   gatherByGid(s, runCommonNeighbors, NULL, &out, 1);
   for (int t = 0; t < 5; ++t) counts[t] = 0;
   for (size_t g = 0; g < n; ++g) { const int t = typeByGid[g]; counts[t >= 0 && t <= 4 ? t : 0] += 1; }
   return 0;
}

/* ---- per-atom virial stress (not in the reference; comd_host.h) ---- */
static void runAtomStress(SimFlat* s, void* const* plane, const void* withKinetic) { computeAtomStress(&s->gpu, *(const int*)withKinetic, (real_t*)plane[0]); }

int comdAtomStress(SimFlat* s, int withKinetic, double* stressByGid)
{
   if (!s->gpu.boxes.nAtoms) return -1;
   const GidOutput out = { stressByGid, SLOT_REAL, 6 };
   gatherByGid(s, runAtomStress, &withKinetic, &out, 1);
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

/* ---- heat flux (not in the reference; comd_host.h) ---- */
int comdHeatFlux(SimFlat* s, double out9[9])
{
   if (!s->gpu.boxes.nAtoms) return -1;
   double local[9];
   computeHeatFlux(&s->gpu, NULL, local);
   startTimer(commReduceTimer);
   addDoubleParallel(local, out9, 9);
   stopTimer(commReduceTimer);
   return 0;
}

static void runAtomHeatFlux(SimFlat* s, void* const* plane, const void* none) { computeHeatFlux(&s->gpu, (real_t*)plane[0], NULL); }

int comdAtomHeatFlux(SimFlat* s, double* byGid)
{
   if (!s->gpu.boxes.nAtoms) return -1;
   const GidOutput out = { byGid, SLOT_REAL, 9 };
   gatherByGid(s, runAtomHeatFlux, NULL, &out, 1);
   return 0;
}

int comdHeatFluxAcf(const double* j, int samples, int window, double* acf)
{
   if (!j || !acf || samples < 1 || window < 1 || window > samples) return -1;
   for (int k = 0; k < window; ++k)
      for (int a = 0; a < 3; ++a) {
         double sum = 0.0;
         for (int t = 0; t + k < samples; ++t) sum += j[3 * (size_t)t + a] * j[3 * (size_t)(t + k) + a];
         acf[3 * (size_t)k + a] = sum / (double)(samples - k);
      }
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
      /* halo neighbours need the records of the other ranks' atoms: every other rank holds 0 for a gid */
      const size_t n = 4 * (size_t)nGlobal;
      double* mine = (double*)malloc(2 * n * sizeof(double));
      double* all = mine + n;
      comdMemcpyDtoH(mine, s->gpu.strainRefBuf, (long)(n * sizeof(double)));
      startTimer(commReduceTimer);
      addDoubleParallelLong(mine, all, n);
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

/* computeAtomStrain picks the image of a reference separation with the box of now (strain_kernels.h) */
static void atomStrainOnTheCurrentBox(SimFlat* s, real_t rCut, real_t* planes, int* counts)
{
   for (int a = 0; a < 3; ++a) s->gpu.strainL[a] = (double)s->domain->globalExtent[a];
   computeAtomStrain(&s->gpu, rCut, planes, counts);
}

static void runAtomStrain(SimFlat* s, void* const* plane, const void* rCut) { atomStrainOnTheCurrentBox(s, *(const real_t*)rCut, (real_t*)plane[0], (int*)plane[1]); }

int comdAtomStrain(SimFlat* s, double rCut, double* strainByGid7, int* countByGid)
{
   rCut = strainRadius(s, rCut);
   if (!(rCut > 0.0)) return -1;
   const real_t r = (real_t)rCut;
   const GidOutput out[2] = { { strainByGid7, SLOT_REAL, 7 }, { countByGid, SLOT_INT, 1 } };
   gatherByGid(s, runAtomStrain, &r, out, 2);
   return 0;
}

int comdStrainSummary(SimFlat* s, double rCut, double threshold, double* out9)
{
   rCut = strainRadius(s, rCut);
   if (!(rCut > 0.0) || !(threshold > 0.0)) return -1;
   double local[9];          /* sum gamma, max gamma, gid, sum vol, sum D^2, max D^2, valid, invalid, above (computeAtomStrainSummary) */
   atomStrainOnTheCurrentBox(s, (real_t)rCut, NULL, NULL);
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

/* ---- Steinhardt's bond-orientational order (not in the reference; comd_host.h) ---- */
static void runSteinhardt(SimFlat* s, void* const* plane, const void* none) { computeSteinhardt(&s->gpu, (real_t*)plane[0]); }

int comdSteinhardt(SimFlat* s, double* outByGid4)
{
   if (!s->gpu.boxes.nAtoms) return -1;
   const GidOutput out = { outByGid4, SLOT_REAL, 4 };
   gatherByGid(s, runSteinhardt, NULL, &out, 1);
   return 0;
}

int comdSteinhardtSummary(SimFlat* s, double threshold, double* out10)
{
   if (!s->gpu.boxes.nAtoms || !(threshold > 0.0 && threshold < 1.0)) return -1;
   double local[10];         /* valid, invalid, sum q4, sum q6, sum w4, sum w6, min q6, gid, max q6, above (computeSteinhardtSummary) */
   computeSteinhardt(&s->gpu, NULL);
   computeSteinhardtSummary(&s->gpu, threshold, local);
   const int nRanks = getNRanks(), me = getMyRank();
   if (nRanks > 1) {
      /* the sums add; the extremes and the gid go through one slot per rank of a summed vector (no MIN/MAX of doubles in the transport), taken in rank order */
      double* mine = (double*)calloc(2 * (size_t)(7 + 3 * nRanks), sizeof(double));
      double* all = mine + 7 + 3 * (size_t)nRanks;
      for (int c = 0; c < 6; ++c) mine[c] = local[c];
      mine[6] = local[9];
      if (local[0] > 0.0) { double* slot = mine + 7 + 3 * (size_t)me; slot[0] = local[6]; slot[1] = local[7] + 1.0; slot[2] = local[8]; }
      startTimer(commReduceTimer);
      addDoubleParallel(mine, all, 7 + 3 * nRanks);
      stopTimer(commReduceTimer);
      for (int c = 0; c < 6; ++c) local[c] = all[c];
      local[9] = all[6];
      local[6] = INFINITY; local[7] = -1.0; local[8] = -INFINITY;
      for (int r = 0; r < nRanks; ++r) {
         const double* slot = all + 7 + 3 * (size_t)r;
         if (slot[1] == 0.0) continue;          /* a rank without valid atoms */
         const double g = slot[1] - 1.0;
         if (local[7] < 0.0 || slot[0] < local[6] || (slot[0] == local[6] && g < local[7])) { local[6] = slot[0]; local[7] = g; }
         if (slot[2] > local[8]) local[8] = slot[2];
      }
      free(mine);
   }
   const double N = local[0];
   out10[0] = N; out10[1] = local[1];
   out10[2] = N > 0.0 ? local[2] / N : 0.0; out10[3] = N > 0.0 ? local[3] / N : 0.0;
   out10[4] = N > 0.0 ? local[6] : 0.0; out10[5] = N > 0.0 ? local[7] : -1.0; out10[6] = N > 0.0 ? local[8] : 0.0;
   out10[7] = N > 0.0 ? local[4] / N : 0.0; out10[8] = N > 0.0 ? local[5] / N : 0.0; out10[9] = local[9];
   return 0;
}

/* ---- the Born matrix and the stress-fluctuation elastic constants (not in the reference; comd_host.h) ---- */
int comdBornMatrix(SimFlat* s, double* born21)
{
   if (!s->gpu.boxes.nAtoms) return -1;
   double local[21];
   computeBornMatrix(&s->gpu, local);
   startTimer(commReduceTimer);
   addDoubleParallel(local, born21, 21);
   stopTimer(commReduceTimer);
   return 0;
}

int comdElasticConstants(const double* bornOverV, const double* stress, int nSamples, double volume, double temperature, double nAtoms, double* outBorn, double* outFluct, double* outKinetic)
{
   if (nSamples < 1 || !(volume >= 0.0) || !(temperature >= 0.0)) return -1;
   double meanS[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
   for (int k = 0; k < nSamples; ++k) for (int i = 0; i < 6; ++i) meanS[i] += stress[6 * (size_t)k + i] / nSamples;
   const int fluctuating = temperature > 0.0 && nSamples >= 2;
   for (int i = 0, c = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j, ++c) {
         double born = 0.0, cov = 0.0;
         for (int k = 0; k < nSamples; ++k) {
            born += bornOverV[21 * (size_t)k + c] / nSamples;
            cov += (stress[6 * (size_t)k + i] - meanS[i]) * (stress[6 * (size_t)k + j] - meanS[j]) / nSamples;          /* <s_I s_J> - <s_I> <s_J>, without its cancellation */
         }
         const double fluct = fluctuating ? -volume / (kB_eV * temperature) * cov : 0.0;
         const double kin = fluctuating && i == j ? (i < 3 ? 2.0 : 1.0) * nAtoms * kB_eV * temperature / volume : 0.0;
         outBorn[6 * i + j] = outBorn[6 * j + i] = born;
         outFluct[6 * i + j] = outFluct[6 * j + i] = fluct;
         outKinetic[6 * i + j] = outKinetic[6 * j + i] = kin;
      }
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
   /* the ranks' parts as doubles (exact below 2^53), summed */
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
      startTimer(commReduceTimer);
      addDoubleParallelLong(mine, out, 3 * n);
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

/* ---- slab profiles (not in the reference; comd_host.h) ---- */
int comdSlabProfile(SimFlat* s, int axis, int nBins, int64_t* out6xN)
{
   if (!s->gpu.boxes.nAtoms || axis < 0 || axis > 2 || nBins < 1 || nBins > COMD_PROFILE_MAX_BINS) return -1;
   computeSlabProfile(&s->gpu, axis, nBins, (double)s->domain->globalExtent[axis], out6xN);
   if (getNRanks() == 1) return 0;
   /* the ranks' words as two 32-bit halves, each exact in a double and in the sum of the ranks' doubles; put together again in integers (mod 2^64, as the device adds) */
   const size_t n = 6 * (size_t)nBins;
   double* mine = (double*)malloc(4 * n * sizeof(double));
   double* all = mine + 2 * n;
   for (size_t k = 0; k < n; ++k) { const uint64_t w = (uint64_t)out6xN[k]; mine[2 * k] = (double)(uint32_t)(w >> 32); mine[2 * k + 1] = (double)(uint32_t)w; }
   startTimer(commReduceTimer);
   addDoubleParallel(mine, all, (int)(2 * n));
   stopTimer(commReduceTimer);
   for (size_t k = 0; k < n; ++k) out6xN[k] = (int64_t)(((uint64_t)all[2 * k] << 32) + (uint64_t)all[2 * k + 1]);
   free(mine);
   return 0;
}

/* ---- Mueller-Plathe exchange (not in the reference; comd_host.h) ---- */
#define MP_ROW 6

int comdMullerPlatheRefusal(int axis, int nBins, int every, int swaps)
{
   if (axis < 0 || axis > 2) return 1;
   if (nBins < 4 || nBins > COMD_PROFILE_MAX_BINS || (nBins & 1)) return 2;
   if (every < 1) return 3;
   if (swaps < 1 || swaps > COMD_MP_MAX_SWAPS) return 4;
   return 0;
}

static double* mpTableOf(SimFlat* s)
{
   if (!s->mpTable) s->mpTable = (double*)malloc(2 * 2 * (size_t)getNRanks() * COMD_MP_MAX_SWAPS * MP_ROW * sizeof(double));
   return s->mpTable;
}

int comdMullerPlatheCandidates(SimFlat* s, int axis, int nBins, int k, double* table)
{
   if (!s->gpu.boxes.nAtoms || comdMullerPlatheRefusal(axis, nBins, 1, k) != 0) return -1;
   const int nRanks = getNRanks(), me = getMyRank();
   const size_t list = (size_t)nRanks * k * MP_ROW, n = 2 * list;
   double local[2 * COMD_MP_MAX_SWAPS * MP_ROW];
   computeMullerPlatheCandidates(&s->gpu, axis, nBins, (double)s->domain->globalExtent[axis], k, local);
   double* mine = nRanks == 1 ? table : mpTableOf(s) + 2 * (size_t)nRanks * COMD_MP_MAX_SWAPS * MP_ROW;
   memset(mine, 0, n * sizeof(double));
   for (int l = 0; l < 2; ++l)
      for (int j = 0; j < k; ++j) {
         const double* rec = local + ((size_t)l * k + j) * MP_ROW;
         if (rec[1] < 0.0) continue;
         double* row = mine + l * list + ((size_t)me * k + j) * MP_ROW;
         memcpy(row, rec, MP_ROW * sizeof(double));
         row[1] = rec[1] + 1.0;
      }
   if (nRanks == 1) return 0;
   startTimer(commReduceTimer);
   addDoubleParallel(mine, table, (int)n);
   stopTimer(commReduceTimer);
   return 0;
}

/* the valid rows of one list in list order, at most k of them: selection by repeated best, the lists are short */
int comdMullerPlatheTop(const double* rows, int nRows, int k, int hot, int* top)
{
   int n = 0;
   for (; n < k; ++n) {
      int best = -1;
      for (int i = 0; i < nRows; ++i) {
         const double* r = rows + (size_t)i * MP_ROW;
         if (r[1] == 0.0) continue;
         int taken = 0;
         for (int t = 0; t < n; ++t) if (top[t] == i) taken = 1;
         if (taken) continue;
         if (best < 0) { best = i; continue; }
         const double* b = rows + (size_t)best * MP_ROW;
         if ((hot ? r[0] < b[0] : r[0] > b[0]) || (r[0] == b[0] && r[1] < b[1])) best = i;
      }
      if (best < 0) break;
      top[n] = best;
   }
   return n;
}

int comdMullerPlatheMatch(const double* cold, int nCold, const double* hot, int nHot, int k, int* pairs, double* deltaE)
{
   *deltaE = 0.0;
   if (k < 1 || nCold < 0 || nHot < 0) return 0;
   int* top = (int*)malloc(2 * (size_t)k * sizeof(int));
   const int nc = comdMullerPlatheTop(cold, nCold, k, 0, top), nh = comdMullerPlatheTop(hot, nHot, k, 1, top + k);
   int kept = 0;
   double sum = 0.0;
   for (; kept < nc && kept < nh; ++kept) {
      const double ka = cold[(size_t)top[kept] * MP_ROW], kb = hot[(size_t)top[k + kept] * MP_ROW];
      if (!(ka > kb)) break;
      pairs[2 * kept] = top[kept]; pairs[2 * kept + 1] = top[k + kept];
      sum += ka - kb;
   }
   *deltaE = sum;
   free(top);
   return kept;
}

int comdMullerPlatheSwap(SimFlat* s, int axis, int nBins, int k, int* pairsGid, double* deltaE, int* skipped)
{
   *deltaE = 0.0; *skipped = 0;
   if (!s->gpu.boxes.nAtoms || comdMullerPlatheRefusal(axis, nBins, 1, k) != 0) return -1;
   const int nRanks = getNRanks(), me = getMyRank();
   double* table = mpTableOf(s);
   comdMullerPlatheCandidates(s, axis, nBins, k, table);
   const double* cold = table;
   const double* hot = table + (size_t)nRanks * k * MP_ROW;
   int pairs[2 * COMD_MP_MAX_SWAPS];
   const int kept = comdMullerPlatheMatch(cold, nRanks * k, hot, nRanks * k, k, pairs, deltaE);
   /* the rows of this rank's atoms: a cold-slab atom takes the momentum of its partner in the hot slab, and the other way round */
   long long slots[2 * COMD_MP_MAX_SWAPS];
   real_t p3[3 * 2 * COMD_MP_MAX_SWAPS];
   int n = 0;
   for (int j = 0; j < kept; ++j) {
      const double* a = cold + (size_t)pairs[2 * j] * MP_ROW;
      const double* b = hot + (size_t)pairs[2 * j + 1] * MP_ROW;
      pairsGid[2 * j] = (int)a[1] - 1; pairsGid[2 * j + 1] = (int)b[1] - 1;
      if (pairs[2 * j] / k == me) { slots[n] = (long long)a[5]; for (int c = 0; c < 3; ++c) p3[3 * n + c] = (real_t)b[2 + c]; n++; }
      if (pairs[2 * j + 1] / k == me) { slots[n] = (long long)b[5]; for (int c = 0; c < 3; ++c) p3[3 * n + c] = (real_t)a[2 + c]; n++; }
   }
   comdMullerPlatheApplyGpu(&s->gpu, n, slots, p3);
   *skipped = k - kept;
   s->mpExchanged += *deltaE; s->mpPairs += kept; s->mpSkipped += k - kept; s->mpExchanges += 1;
   return kept;
}

int comdFourierKappa(const double* T, int nBins, double width, double area, double energy, double time, double* gradient, double* kappa)
{
   if (nBins < 2 || (nBins & 1)) return -1;
   const int half = nBins / 2;
   int n = 0;
   double mx = 0.0, my = 0.0;
   for (int b = 1; b < half; ++b) {
      const double t = 0.5 * (T[b] + T[nBins - b]);
      if (!(t == t)) continue;
      mx += (double)b * width; my += t; n++;
   }
   if (n < 2) return -1;
   mx /= n; my /= n;
   double sxx = 0.0, sxy = 0.0;
   for (int b = 1; b < half; ++b) {
      const double t = 0.5 * (T[b] + T[nBins - b]);
      if (!(t == t)) continue;
      const double dx = (double)b * width - mx;
      sxx += dx * dx; sxy += dx * (t - my);
   }
   if (!(sxx > 0.0)) return -1;
   const double g = fabs(sxy / sxx);
   *gradient = g;
   if (!(g > 0.0) || !(area > 0.0) || !(time > 0.0)) return 1;
   *kappa = energy / (2.0 * area * time) / g * 1.602176634e6;
   return 0;
}

/* ---- static structure factor (not in the reference; comd_host.h) ---- */
int comdStructureFactorRefusal(int M, const int stride[3])
{
   if (M < 1 || M > COMD_SK_MAX_M) return 1;
   for (int a = 0; a < 3; ++a) if (stride[a] < 1) return 2;
   for (int a = 0; a < 3; ++a) if ((long long)stride[a] * M > COMD_SK_MAX_HM) return 3;
   return 0;
}

int comdStructureFactor(SimFlat* s, int M, const int stride[3], double* outKx2)
{
   const int why = comdStructureFactorRefusal(M, stride);
   if (why) return why;
   if (!s->gpu.boxes.nAtoms) return -1;
   const double extent[3] = { (double)s->domain->globalExtent[0], (double)s->domain->globalExtent[1], (double)s->domain->globalExtent[2] };
   computeStructureFactor(&s->gpu, M, stride, extent, outKx2);
   if (getNRanks() == 1) return 0;
   const size_t n = (size_t)2 * (M + 1) * (2 * M + 1) * (2 * M + 1);
   double* mine = (double*)malloc(n * sizeof(double));
   memcpy(mine, outKx2, n * sizeof(double));
   startTimer(commReduceTimer);
   addDoubleParallelLong(mine, outKx2, n);
   stopTimer(commReduceTimer);
   free(mine);
   return 0;
}

#define SK_TWO_PI 6.283185307179586

int comdStructureFactorRadial(const double* rhoKx2, int M, const int stride[3], const double box[3], int nBins, double* kCentre, double* sMean, double* count)
{
   const int why = comdStructureFactorRefusal(M, stride);
   if (why) return why;
   if (nBins < 1 || nBins > COMD_SK_MAX_BINS) return 4;
   const int W = 2 * M + 1;
   const double nAtoms = rhoKx2[2 * ((size_t)M * W + M)];      /* rho(0, 0, 0) */
   for (int a = 0; a < 3; ++a) if (!(box[a] > 0.0) || !(box[a] < INFINITY)) return 5;
   if (!(nAtoms > 0.0) || !(nAtoms < INFINITY)) return 5;
   double kMax = INFINITY;
   for (int a = 0; a < 3; ++a) { const double k = (SK_TWO_PI * (double)(stride[a] * M)) / box[a]; if (k < kMax) kMax = k; }
   const double dk = kMax / nBins;
   for (int b = 0; b < nBins; ++b) { kCentre[b] = (b + 0.5) * dk; sMean[b] = 0.0; count[b] = 0.0; }
   for (int h = 0; h <= M; ++h)
      for (int k = -M; k <= M; ++k)
         for (int l = -M; l <= M; ++l) {
            if (h == 0 && k == 0 && l == 0) continue;
            const double kx = (SK_TWO_PI * (double)(stride[0] * h)) / box[0], ky = (SK_TWO_PI * (double)(stride[1] * k)) / box[1], kz = (SK_TWO_PI * (double)(stride[2] * l)) / box[2];
            const double kk = sqrt((kx * kx + ky * ky) + kz * kz);
            if (!(kk <= kMax)) continue;
            int b = (int)floor(kk / dk);
            if (b > nBins - 1) b = nBins - 1;
            const double* r = rhoKx2 + 2 * (((size_t)h * W + (k + M)) * W + (l + M));
            const double weight = h > 0 ? 2.0 : 1.0;
            sMean[b] += weight * ((r[0] * r[0] + r[1] * r[1]) / nAtoms);
            count[b] += weight;
         }
   for (int b = 0; b < nBins; ++b) sMean[b] = count[b] > 0.0 ? sMean[b] / count[b] : NAN;
   return 0;
}

int comdBraggOrder(SimFlat* s, double* out)
{
   double rho[2 * 2 * 3 * 3];
   const int rc = comdStructureFactor(s, 1, s->cells, rho);
   if (rc != 0) return -1;
   const double nAtoms = rho[2 * (1 * 3 + 1)];
   double sum = 0.0;
   for (int k = 0; k < 3; k += 2)
      for (int l = 0; l < 3; l += 2) { const double* r = rho + 2 * ((3 + k) * 3 + l); sum += (r[0] * r[0] + r[1] * r[1]) / nAtoms; }      /* h = 1 */
   *out = (sum / 4.0) / nAtoms;
   return 0;
}
