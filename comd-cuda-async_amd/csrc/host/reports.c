/* reports.c -- the run-time reports of the driver (none is in the reference): what each one samples at a printed step, the column it shows in printThings, and
 * the files and the YAML block it writes at the end of the run.  The table at the end of the file is all that comdMain and printThings know about them. */
#include "comd_host.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

/* the next row of a table of samples that grows by doubling */
void* nextRow(RowTable* t, size_t rowBytes)
{
   if (t->n == t->cap) { t->cap = t->cap ? 2 * t->cap : 64; t->rows = realloc(t->rows, (size_t)t->cap * rowBytes); }
   return (char*)t->rows + rowBytes * (size_t)t->n++;
}

/* a file a report writes, on the print rank */
static FILE* openReport(const char* path)
{
   FILE* f = fopen(path, "w");
   if (!f) { printf("Error: cannot write %s\n", path); exit(-1); }
   return f;
}

/* a row of a file: the step, then the other values to 17 digits */
static void printRow(FILE* f, const double* r, int width) { fprintf(f, "%.0f", r[0]); for (int c = 1; c < width; ++c) fprintf(f, " %.17g", r[c]); fprintf(f, "\n"); }

/* --pressure, and every report that reads W, K, V: they are the current state's before any sampler runs */
static void samplePressure(SimFlat* s, int iStep) { computePressure(s); }

/* --pressure: the final pressure and tensor (K + W) / V, components xx yy zz yz xz xy */
static void writePressure(FILE* file, SimFlat* s, int iStep)
{
   if (!printRank() || !file) return;
   static const char* name[6] = { "xx", "yy", "zz", "yz", "xz", "xy" };
   fprintf(file, "Pressure:\n  Units: GPa\n  Pressure: %.12e\n", pressureOf(s) * eVperA3inGPa);
   for (int c = 0; c < 6; ++c) fprintf(file, "  P%s: %.12e\n", name[c], ((double)s->K[c] + s->W[c]) / s->V * eVperA3inGPa);
   fprintf(file, "\n");
}

/* --rdf: one more sample of the global pair histogram into rdfSum */
static void sampleRdf(SimFlat* s, int iStep)
{
   double* counts = (double*)malloc((size_t)s->rdfBins * sizeof(double));
   if (comdPairHistogram(s, s->rdfBins, s->rdfMax, counts) != 0) { printf("Error: --rdf %d --rdfMax %g was refused.\n", s->rdfBins, s->rdfMax); exit(-1); }
   for (int k = 0; k < s->rdfBins; ++k) s->rdfSum[k] += counts[k];
   s->rdfDensitySum += (double)s->atoms->nGlobal / ((double)s->domain->globalExtent[0] * s->domain->globalExtent[1] * s->domain->globalExtent[2]);
   s->rdfSamples++;
   free(counts);
}

/* --rdf: g_k = counts_k / (samples (N/2) (N/V) (4 pi/3) ((k + 1)^3 - k^3) dr^3), the ideal-gas count of unordered pairs in the shell of bin k; with a box
 * that changed during the run (--erateX/Y/Z) N/V is the mean over the samples, and the header's V is N over that mean.
 * The file: a header line, then per bin its centre, g, the running coordination number n(r) = 2 sum counts / (samples N) up to the bin's upper edge and the
 * mean pair count per sample.  The YAML block names the file and the position of the highest peak. */
static void writeRdf(FILE* yaml, SimFlat* s, int iStep)
{
   if (!printRank()) return;
   const int nBins = s->rdfBins, samples = s->rdfSamples;
   const double N = (double)s->atoms->nGlobal;
   const double V = s->boxChanged && samples > 0 ? N / (s->rdfDensitySum / samples) : (double)s->domain->globalExtent[0] * s->domain->globalExtent[1] * s->domain->globalExtent[2];
   const double dr = s->rdfMax / nBins, shell = 4.0 * M_PI / 3.0 * dr * dr * dr;
   FILE* f = openReport(s->rdfFile);
   fprintf(f, "# g(r): bins %d rMax %.17g samples %d N %d V %.17g | columns: r (A), g(r), n(r), pairs per sample\n", nBins, s->rdfMax, samples, s->atoms->nGlobal, V);
   double running = 0.0, gTop = -1.0, rTop = 0.0;
   for (int k = 0; k < nBins; ++k) {
      const double k0 = (double)k, k1 = (double)k + 1.0;
      const double g = s->rdfSum[k] / ((double)samples * (0.5 * N) * (N / V) * shell * (k1 * k1 * k1 - k0 * k0 * k0));
      running += s->rdfSum[k];
      fprintf(f, "%.17g %.17g %.17g %.17g\n", (k0 + 0.5) * dr, g, 2.0 * running / ((double)samples * N), s->rdfSum[k] / (double)samples);
      if (g > gTop) { gTop = g; rTop = (k0 + 0.5) * dr; }
   }
   fclose(f);
   if (yaml) fprintf(yaml, "RDF:\n  bins: %d\n  rMax: %.12e\n  samples: %d\n  file: %s\n  rOfHighestG: %.12e\n\n", nBins, s->rdfMax, samples, s->rdfFile, rTop);
}

/* --msd: the origin: tracking on (or, were it on already, zeroed again) */
static void startMsd(SimFlat* s)
{
   if (comdTrackDisplacement(s, 1) != 0) { printf("Error: --msd: no device memory for the displacement records of %d atoms.\n", s->atoms->nGlobal); exit(-1); }
}

/* positions by gid over all ranks, [nGlobal][3], malloc'd: collective */
static double* positionsByGid(SimFlat* s)
{
   const size_t n = (size_t)s->atoms->nGlobal;
   double* mine = (double*)calloc(n ? 3 * n : 1, sizeof(double));
   double* pos = (double*)malloc((n ? 3 * n : 1) * sizeof(double));
   comdGatherByGid(s, 0, mine);
   addDoubleParallelLong(mine, pos, 3 * n);
   free(mine);
   return pos;
}

/* an extended-XYZ dump (--cspDump, --cnaDump, --stressDump, --strainDump, --stDump) of the atoms `row` keeps: their number, the Lattice= line of the current box with the
 * caller's properties and settings behind species and pos, then per kept atom "Cu x y z" and what row(f, g, ctx) prints behind it; row(NULL, g, ctx) only
 * says whether atom g is kept.  On the print rank, with the positions of positionsByGid */
typedef int (*XyzRow)(FILE* f, size_t g, const void* ctx);
static void writeXyz(const char* path, const SimFlat* s, const double* pos, const char* tail, XyzRow row, const void* ctx)
{
   FILE* f = openReport(path);
   const size_t n = (size_t)s->atoms->nGlobal;
   const real_t* L = s->domain->globalExtent;
   size_t kept = 0;
   for (size_t g = 0; g < n; ++g) kept += (size_t)row(NULL, g, ctx);
   fprintf(f, "%zu\n", kept);
   fprintf(f, "Lattice=\"%.17g 0 0 0 %.17g 0 0 0 %.17g\" Properties=species:S:1:pos:R:3:%s\n", (double)L[0], (double)L[1], (double)L[2], tail);
   for (size_t g = 0; g < n; ++g)
      if (row(NULL, g, ctx)) { fprintf(f, "Cu %.17g %.17g %.17g", pos[3 * g], pos[3 * g + 1], pos[3 * g + 2]); row(f, g, ctx); }
   fclose(f);
}

/* --msd: one more row {step, sum d (3), sum d^2 (3), N} */
static void sampleMsd(SimFlat* s, int iStep)
{
   double* row = (double*)nextRow(&s->msdRows, 8 * sizeof(double));
   row[0] = (double)iStep;
   if (comdMsd(s, row + 1) != 0) { printf("Error: --msd: the displacements could not be summed.\n"); exit(-1); }
   s->msdNow = (row[4] + row[5] + row[6]) / row[7];
}

/* --msd: the file: a header line, then per sample the time since the origin in fs, MSD = sum |d|^2 / N, its x, y, z parts and the MSD with the drift of the
 * centre of mass removed, sum |d|^2 / N - |sum d / N|^2 (a Langevin thermostat does not conserve momentum: the centre of mass walks).  The YAML block names
 * the file and gives D = slope / 6 of a least-squares line through the drift-removed MSD of the samples in the second half of the tracked interval. */
static void writeMsd(FILE* yaml, SimFlat* s, int iStep)
{
   if (!printRank()) return;
   const int samples = s->msdRows.n;
   const double* rows = (const double*)s->msdRows.rows;
   FILE* f = openReport(s->msdFile);
   fprintf(f, "# MSD: N %d dt %.17g originStep %d samples %d | columns: t - t0 (fs), MSD (A^2), MSD_x, MSD_y, MSD_z, MSD without the centre-of-mass drift\n",
           s->atoms->nGlobal, s->dt, s->msdStart, samples);
   double tLast = 0.0, msdLast = 0.0, freeLast = 0.0;
   double st = 0.0, sy = 0.0, stt = 0.0, sty = 0.0; int m = 0;
   if (samples > 0) tLast = (rows[8 * (size_t)(samples - 1)] - s->msdStart) * s->dt;
   for (int k = 0; k < samples; ++k) {
      const double* row = rows + 8 * (size_t)k;
      const double N = row[7], t = (row[0] - s->msdStart) * s->dt;
      const double mx = row[4] / N, my = row[5] / N, mz = row[6] / N;
      const double cx = row[1] / N, cy = row[2] / N, cz = row[3] / N;
      msdLast = mx + my + mz; freeLast = msdLast - (cx * cx + cy * cy + cz * cz);
      fprintf(f, "%.17g %.17g %.17g %.17g %.17g %.17g\n", t, msdLast, mx, my, mz, freeLast);
      if (t >= 0.5 * tLast) { st += t; sy += freeLast; stt += t * t; sty += t * freeLast; m++; }
   }
   fclose(f);
   if (!yaml) return;
   fprintf(yaml, "MSD:\n  originStep: %d\n  samples: %d\n  finalMSD: %.12e\n  finalMSDNoDrift: %.12e\n  Units: Angstroms^2\n  file: %s\n",
           s->msdStart, samples, msdLast, freeLast, s->msdFile);
   const double det = m * stt - st * st;
   if (m >= 3 && det > 0.0) {
      const double D = (m * sty - st * sy) / det / 6.0;
      fprintf(yaml, "  D: %.12e\n  DUnits: Angstroms^2/fs\n  D_cm2_per_s: %.12e\n  fitSamples: %d\n", D, 0.1 * D, m);
   } else fprintf(yaml, "  D: n/a\n");
   fprintf(yaml, "\n");
}

/* --csp: one more row {step, defects, atoms with fewer than 12 neighbours, mean and max of the finite csp, mean coordination, atoms with coordination != 12} */
static void sampleCsp(SimFlat* s, int iStep)
{
   const size_t n = (size_t)s->atoms->nGlobal;
   if (!s->cspLast) s->cspLast = (double*)malloc((n ? 2 * n : 1) * sizeof(double));
   if (comdCentroSymmetry(s, s->cspCoord, s->cspLast, s->cspLast + n) != 0) { printf("Error: --csp --cspCoord %g was refused.\n", s->cspCoord); exit(-1); }
   double* row = (double*)nextRow(&s->cspRows, 7 * sizeof(double));
   double defects = 0.0, few = 0.0, sum = 0.0, top = 0.0, coordSum = 0.0, not12 = 0.0;
   for (size_t g = 0; g < n; ++g) {
      const double c = s->cspLast[g], z = s->cspLast[n + g];
      if (c > s->cspThreshold) defects += 1.0;
      if (isinf(c)) few += 1.0; else { sum += c; if (c > top) top = c; }
      coordSum += z;
      if (z != 12.0) not12 += 1.0;
   }
   row[0] = (double)iStep; row[1] = defects; row[2] = few;
   row[3] = n > few ? sum / ((double)n - few) : 0.0; row[4] = top;
   row[5] = n ? coordSum / (double)n : 0.0; row[6] = not12;
   s->cspDefectsNow = (int)defects;
}

/* --csp: the file: a header line, then the rows of sampleCsp.  --cspDump: the defect atoms of the last sample as extended XYZ, Cu x y z csp coordination gid,
 * the positions gathered by gid over the ranks as the results are.  The YAML block names the file and gives the last sample's defects and mean csp. */
static int cspXyzRow(FILE* f, size_t g, const void* ctx)
{
   const SimFlat* s = (const SimFlat*)ctx;
   if (f) fprintf(f, " %.17g %d %zu\n", s->cspLast[g], (int)s->cspLast[(size_t)s->atoms->nGlobal + g], g);
   return s->cspLast[g] > s->cspThreshold;
}

static void writeCsp(FILE* yaml, SimFlat* s, int iStep)
{
   double* pos = s->cspDump[0] ? positionsByGid(s) : NULL;          /* collective: before the other ranks leave */
   if (!printRank()) { free(pos); return; }
   const int samples = s->cspRows.n;
   const double* rows = (const double*)s->cspRows.rows;
   FILE* f = openReport(s->cspFile);
   fprintf(f, "# CSP: N %d threshold %.17g rCoord %.17g samples %d | columns: step, defects (csp > threshold), atoms with fewer than 12 neighbours, "
              "mean csp (A^2, finite ones), max csp, mean coordination, atoms with coordination != 12\n", s->atoms->nGlobal, s->cspThreshold, s->cspCoord, samples);
   const double* last = NULL;
   for (int k = 0; k < samples; ++k) {
      last = rows + 7 * (size_t)k;
      fprintf(f, "%.0f %.0f %.0f %.17g %.17g %.17g %.0f\n", last[0], last[1], last[2], last[3], last[4], last[5], last[6]);
   }
   fclose(f);
   if (pos && s->cspLast) {
      char tail[256];
      snprintf(tail, sizeof tail, "csp:R:1:coordination:I:1:gid:I:1 step=%.0f threshold=%.17g rCoord=%.17g", last ? last[0] : 0.0, s->cspThreshold, s->cspCoord);
      writeXyz(s->cspDump, s, pos, tail, cspXyzRow, s);
   }
   free(pos);
   if (yaml) fprintf(yaml, "CSP:\n  threshold: %.12e\n  rCoord: %.12e\n  samples: %d\n  file: %s\n  finalDefects: %.0f\n  finalMeanCsp: %.12e\n\n",
           s->cspThreshold, s->cspCoord, samples, s->cspFile, last ? last[1] : 0.0, last ? last[3] : 0.0);
}

/* --cna: one more row {step, atoms of type OTHER, FCC, HCP, ICO} */
static void sampleCna(SimFlat* s, int iStep)
{
   const size_t n = (size_t)s->atoms->nGlobal;
   if (!s->cnaLast) s->cnaLast = (int*)malloc((n ? n : 1) * sizeof(int));
   long long counts[5];
   comdCommonNeighbors(s, s->cnaLast, counts);
   long long* row = (long long*)nextRow(&s->cnaRows, 5 * sizeof(long long));
   row[0] = iStep; row[1] = counts[COMD_CNA_OTHER]; row[2] = counts[COMD_CNA_FCC]; row[3] = counts[COMD_CNA_HCP]; row[4] = counts[COMD_CNA_ICO];
   s->cnaNonFccNow = (long long)n - counts[COMD_CNA_FCC];
}

/* --cna: the file: a header line, then the rows of sampleCna.  --cnaDump: the non-FCC atoms of the last sample as extended XYZ, Cu x y z type gid, the
 * positions gathered by gid over the ranks as the types are.  The YAML block names the file and gives the last sample's counts and HCP fraction. */
static int cnaXyzRow(FILE* f, size_t g, const void* ctx)
{
   const SimFlat* s = (const SimFlat*)ctx;
   if (f) fprintf(f, " %d %zu\n", s->cnaLast[g], g);
   return s->cnaLast[g] != COMD_CNA_FCC;
}

static void writeCna(FILE* yaml, SimFlat* s, int iStep)
{
   const size_t n = (size_t)s->atoms->nGlobal;
   double* pos = s->cnaDump[0] ? positionsByGid(s) : NULL;          /* collective: before the other ranks leave */
   if (!printRank()) { free(pos); return; }
   const int samples = s->cnaRows.n;
   const long long* rows = (const long long*)s->cnaRows.rows;
   FILE* f = openReport(s->cnaFile);
   fprintf(f, "# CNA: N %d samples %d | columns: step, atoms of type other (0), FCC (1), HCP (2), ICO (4)\n", s->atoms->nGlobal, samples);
   const long long zero[5] = { 0, 0, 0, 0, 0 };
   const long long* last = zero;
   for (int k = 0; k < samples; ++k) {
      last = rows + 5 * (size_t)k;
      fprintf(f, "%lld %lld %lld %lld %lld\n", last[0], last[1], last[2], last[3], last[4]);
   }
   fclose(f);
   if (pos && s->cnaLast) {
      char tail[64];
      snprintf(tail, sizeof tail, "type:I:1:gid:I:1 step=%lld", last[0]);
      writeXyz(s->cnaDump, s, pos, tail, cnaXyzRow, s);
   }
   free(pos);
   if (yaml) fprintf(yaml, "CNA:\n  samples: %d\n  file: %s\n  finalOther: %lld\n  finalFCC: %lld\n  finalHCP: %lld\n  finalICO: %lld\n  finalHCPFraction: %.12e\n\n",
           samples, s->cnaFile, last[1], last[2], last[3], last[4], n ? (double)last[3] / (double)n : 0.0);
}

/* --erateX/Y/Z: one more row {step, time, strain (3), extents (3), volume, stress = -(K + W) / V in GPa (xx yy zz yz xz xy; tension positive), temperature} from
 * the tensors computePressure has just left in W, K, V */
static void sampleDeform(SimFlat* s, int iStep)
{
   double* row = (double*)nextRow(&s->deformRows, 15 * sizeof(double));
   row[0] = (double)iStep; row[1] = iStep * s->dt;
   for (int a = 0; a < 3; ++a) { row[5 + a] = (double)s->domain->globalExtent[a]; row[2 + a] = row[5 + a] / s->box0[a] - 1.0; }
   row[8] = (double)s->V;
   for (int c = 0; c < 6; ++c) row[9 + c] = -((double)s->K[c] + s->W[c]) / s->V * eVperA3inGPa;
   row[14] = (s->eKinetic / s->atoms->nGlobal) / (kB_eV * 1.5);
}

/* --erateX/Y/Z: the file: a header with N, the initial box and the rates, then the rows of sampleDeform.  The YAML block gives the rates, the start step, the
 * final strains and box, the file and the number of samples. */
static void writeDeform(FILE* yaml, SimFlat* s, int iStep)
{
   if (!printRank()) return;
   const int samples = s->deformRows.n;
   const double* rows = (const double*)s->deformRows.rows;
   FILE* f = openReport(s->deformFile);
   fprintf(f, "# Deform: N %d L0 %.17g %.17g %.17g rates(1/ps) %.17g %.17g %.17g startStep %d samples %d | columns: step, time (fs), strain x y z, L x y z (A), V (A^3), "
              "stress xx yy zz yz xz xy (GPa, tension positive), T (K)\n",
           s->atoms->nGlobal, s->box0[0], s->box0[1], s->box0[2], s->erate[0], s->erate[1], s->erate[2], s->deformStart, samples);
   for (int k = 0; k < samples; ++k) printRow(f, rows + 15 * (size_t)k, 15);
   fclose(f);
   if (!yaml) return;
   const real_t* L = s->domain->globalExtent;
   fprintf(yaml, "Deform:\n  rates: [ %.12e, %.12e, %.12e ]\n  rateUnits: 1/ps\n  startStep: %d\n", s->erate[0], s->erate[1], s->erate[2], s->deformStart);
   fprintf(yaml, "  finalStrain: [ %.12e, %.12e, %.12e ]\n", (double)L[0] / s->box0[0] - 1.0, (double)L[1] / s->box0[1] - 1.0, (double)L[2] / s->box0[2] - 1.0);
   fprintf(yaml, "  finalBox: [ %.12e, %.12e, %.12e ]\n  file: %s\n  samples: %d\n\n", (double)L[0], (double)L[1], (double)L[2], s->deformFile, samples);
}

/* --baro: the file: a header with the settings, then the rows timestep() has kept, one per coupling.  The YAML block gives the settings, the couplings, the final
 * box and the mean of the fast pressure over the last half of the couplings. */
static void writeBaro(FILE* yaml, SimFlat* s, int iStep)
{
   if (!printRank()) return;
   const int n = s->baroRows.n;
   const double* rows = (const double*)s->baroRows.rows;
   char axes[4] = "", *c = axes;
   for (int a = 0; a < 3; ++a) if (s->baroAxes >> a & 1) *c++ = (char)('x' + a);
   *c = '\0';
   FILE* f = openReport(s->baroFile);
   fprintf(f, "# Barostat: N %d target(GPa) %.17g tau(fs) %.17g modulus(GPa) %.17g every %d axes %s iso %d startStep %d couplings %d | columns: step, time (fs), "
              "p xx yy zz (GPa, compressive positive, from the forces and the face pairs), mu x y z, L x y z (A) and V (A^3) the coupling asked for\n",
           s->atoms->nGlobal, s->baroTarget[0], s->baroTau, s->baroModulus, s->baroEvery, axes, s->baroIso, s->baroStart, n);
   for (int k = 0; k < n; ++k) printRow(f, rows + 12 * (size_t)k, 12);
   fclose(f);
   if (!yaml) return;
   double mean[3] = { 0.0, 0.0, 0.0 };
   const int from = n / 2;
   for (int k = from; k < n; ++k) for (int a = 0; a < 3; ++a) mean[a] += rows[12 * (size_t)k + 2 + a] / (double)(n - from);
   const real_t* L = s->domain->globalExtent;
   fprintf(yaml, "Barostat:\n  target: %.12e\n  pressureUnits: GPa\n  tau: %.12e\n  modulus: %.12e\n  every: %d\n  axes: %s\n  iso: %d\n  startStep: %d\n",
           s->baroTarget[0], s->baroTau, s->baroModulus, s->baroEvery, axes, s->baroIso, s->baroStart);
   fprintf(yaml, "  couplings: %d\n  finalBox: [ %.12e, %.12e, %.12e ]\n", n, (double)L[0], (double)L[1], (double)L[2]);
   fprintf(yaml, "  meanPressureLastHalf: [ %.12e, %.12e, %.12e ]\n  file: %s\n\n", mean[0], mean[1], mean[2], s->baroFile);
}

/* --profile: the planes of this printed step are added to the sums; integers, so the time average does not depend on the order either */
static void sampleProfile(SimFlat* s, int iStep)
{
   const int n = s->profBins;
   int64_t* now = (int64_t*)malloc(6 * (size_t)n * sizeof(int64_t));
   if (comdSlabProfile(s, s->profAxis, n, now) != 0) { printf("Error: --profile needs the device state.\n"); exit(-1); }
   for (int k = 0; k < 6 * n; ++k) s->profSum[k] += now[k];
   free(now);
   const real_t* L = s->domain->globalExtent;
   if (s->profSamples == 0) s->profFirstStep = iStep;
   s->profLastStep = iStep;
   s->profSamples++;
   s->profLSum += (double)L[s->profAxis];
   s->profAreaSum += (double)L[(s->profAxis + 1) % 3] * (double)L[(s->profAxis + 2) % 3];
}

#define COMD_PROFILE_UNIT (1.0 / 4294967296.0)      /* eV, eV fs/A per unit of the device sums */

/* --profile, --mp: the files and the YAML blocks.  profFile: a header with N, the axis, the bins, the mean extent and the samples, then per bin the centre (A), the
 * mean count per sample, the time-averaged temperature T = 2 sum KE / (3 kB sum count) (K), the mean KE and e per atom (eV) and the mean velocity x y z (A/fs); an
 * empty bin prints nan.  mpFile: a row per exchange.  The conductivity: q = E / (2 A t) with E the energy exchanged since global step profStart (the exchanges
 * of the steps after it) and t the time from that step to the last sample, A the mean cross-section, the gradient from comdFourierKappa. */
static void writeProfile(FILE* yaml, SimFlat* s, int iStep)
{
   if (!printRank()) return;
   const int n = s->profBins, samples = s->profSamples;
   const double meanL = samples ? s->profLSum / samples : (double)s->domain->globalExtent[s->profAxis], width = meanL / n;
   const double mass = (double)s->species[0].mass;
   double* T = (double*)malloc((size_t)n * sizeof(double));
   double tMin = NAN, tMax = NAN;
   FILE* f = openReport(s->profFile);
   fprintf(f, "# Profile: N %d axis %c bins %d meanL %.17g A samples %d startStep %d | columns: bin centre (A), mean count per sample, T (K), KE per atom (eV), "
              "e per atom (eV), mean velocity x y z (A/fs)\n", s->atoms->nGlobal, 'x' + s->profAxis, n, meanL, samples, s->profStart);
   for (int b = 0; b < n; ++b) {
      const double count = (double)s->profSum[b];
      if (count > 0.0) {
         const double ke = (double)s->profSum[4 * n + b] * COMD_PROFILE_UNIT;
         T[b] = 2.0 * ke / (3.0 * kB_eV * count);
         if (!(tMin <= T[b])) tMin = T[b];
         if (!(tMax >= T[b])) tMax = T[b];
         fprintf(f, "%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", (b + 0.5) * width, count / samples, T[b], ke / count,
                 (double)s->profSum[5 * n + b] * COMD_PROFILE_UNIT / count, (double)s->profSum[n + b] * COMD_PROFILE_UNIT / count / mass,
                 (double)s->profSum[2 * n + b] * COMD_PROFILE_UNIT / count / mass, (double)s->profSum[3 * n + b] * COMD_PROFILE_UNIT / count / mass);
      } else {
         T[b] = NAN;
         fprintf(f, "%.17g %.17g nan nan nan nan nan nan\n", (b + 0.5) * width, 0.0);
      }
   }
   fclose(f);
   if (yaml) {
      fprintf(yaml, "Profile:\n  axis: %c\n  bins: %d\n  startStep: %d\n  samples: %d\n  file: %s\n", 'x' + s->profAxis, n, s->profStart, samples, s->profFile);
      if (tMin == tMin) fprintf(yaml, "  minTemperature: %.12e\n  maxTemperature: %.12e\n", tMin, tMax); else fprintf(yaml, "  minTemperature: n/a\n  maxTemperature: n/a\n");
      fprintf(yaml, "  temperatureUnits: K\n\n");
   }
   if (s->mpReport) {
      f = openReport(s->mpFile);
      fprintf(f, "# MullerPlathe: N %d axis %c bins %d every %d swaps %d startStep %d exchanges %d | columns: step, time (fs), kept pairs, skipped pairs, dE (eV), "
                 "cumulative E (eV)\n", s->atoms->nGlobal, 'x' + s->mpAxis, s->mpBins, s->mpEvery, s->mpSwaps, s->mpStart, s->mpRows.n);
      for (int k = 0; k < s->mpRows.n; ++k) {
         const double* r = (const double*)s->mpRows.rows + 6 * (size_t)k;
         fprintf(f, "%.0f %.17g %.0f %.0f %.17g %.17g\n", r[0], r[1], r[2], r[3], r[4], r[5]);
      }
      fclose(f);
      if (yaml) {
         const double E = s->mpExchanged - s->mpExchangedAtProfStart, time = samples ? (double)(s->profLastStep - s->profStart) * s->dt : 0.0;
         const double area = samples ? s->profAreaSum / samples : 0.0;
         double gradient = 0.0, kappa = 0.0;
         const int rc = samples >= 2 ? comdFourierKappa(T, n, width, area, E, time, &gradient, &kappa) : -1;
         fprintf(yaml, "MullerPlathe:\n  axis: %c\n  bins: %d\n  every: %d\n  swaps: %d\n  startStep: %d\n  file: %s\n", 'x' + s->mpAxis, s->mpBins, s->mpEvery, s->mpSwaps, s->mpStart, s->mpFile);
         fprintf(yaml, "  exchanges: %lld\n  keptPairs: %lld\n  skippedPairs: %lld\n  exchangedSinceProfStart: %.12e\n  energyUnits: eV\n", s->mpExchanges, s->mpPairs, s->mpSkipped, E);
         if (time > 0.0 && area > 0.0) fprintf(yaml, "  heatFlux: %.12e\n", E / (2.0 * area * time)); else fprintf(yaml, "  heatFlux: n/a\n");
         fprintf(yaml, "  heatFluxUnits: eV/A^2/fs\n");
         if (rc >= 0) fprintf(yaml, "  gradient: %.12e\n", gradient); else fprintf(yaml, "  gradient: n/a\n");
         fprintf(yaml, "  gradientUnits: K/A\n");
         if (rc == 0) fprintf(yaml, "  kappa: %.12e\n", kappa); else fprintf(yaml, "  kappa: n/a\n");
         fprintf(yaml, "  kappaUnits: W/m/K\n\n");
      }
   }
   free(T);
}

/* --stress: one more row {step, mean / min / max hydrostatic pressure, mean / max von Mises stress, the gid of the max, N} from the device reduction (eV/A^3) */
static void sampleStress(SimFlat* s, int iStep)
{
   double* row = (double*)nextRow(&s->stressRows, 8 * sizeof(double));
   row[0] = (double)iStep;
   if (comdStressSummary(s, 1, row + 1) != 0) { printf("Error: --stress needs the device state.\n"); exit(-1); }
   s->stressMaxVmNow = row[5];
}

/* --stress: the file: a header line, then the rows of sampleStress in GPa.  --stressDump: the tensors of the last step as extended XYZ, Cu x y z sxx syy szz syz
 * sxz sxy vm gid in GPa (the tensor over the uniform atomic volume), the atoms whose von Mises stress is at least --stressDumpMin; the positions gathered by gid
 * over the ranks as the tensors are.  The YAML block names the file and gives the last sample's mean pressure and mean and max von Mises stress. */
typedef struct { const double* ten; double toGPa, min; } StressDump;
static int stressXyzRow(FILE* f, size_t g, const void* ctx)
{
   const StressDump* d = (const StressDump*)ctx;
   const double *t = d->ten + 6 * g, toGPa = d->toGPa;
   const double d0 = t[0] - t[1], d1 = t[1] - t[2], d2 = t[2] - t[0];
   const double vm = sqrt(0.5 * ((d0 * d0 + d1 * d1) + d2 * d2) + 3.0 * ((t[3] * t[3] + t[4] * t[4]) + t[5] * t[5])) * toGPa;
   if (f) fprintf(f, " %.17g %.17g %.17g %.17g %.17g %.17g %.17g %zu\n", t[0] * toGPa, t[1] * toGPa, t[2] * toGPa, t[3] * toGPa, t[4] * toGPa, t[5] * toGPa, vm, g);
   return vm >= d->min;
}

static void writeStress(FILE* yaml, SimFlat* s, int iStep)
{
   const size_t n = (size_t)s->atoms->nGlobal;
   const double omega = (double)s->domain->globalExtent[0] * s->domain->globalExtent[1] * s->domain->globalExtent[2] / (n ? (double)n : 1.0);
   double *pos = NULL, *ten = NULL;
   if (s->stressDump[0]) {          /* collective: before the other ranks leave */
      pos = positionsByGid(s);
      ten = (double*)malloc((n ? 6 * n : 1) * sizeof(double));
      if (comdAtomStress(s, 1, ten) != 0) { printf("Error: --stressDump needs the device state.\n"); exit(-1); }
   }
   if (!printRank()) { free(pos); free(ten); return; }
   const int samples = s->stressRows.n;
   const double* rows = (const double*)s->stressRows.rows;
   FILE* f = openReport(s->stressFile);
   fprintf(f, "# Stress: N %d atomic volume %.17g A^3 (V / N of the last sample) samples %d | columns: step, mean / min / max hydrostatic pressure (GPa), "
              "mean / max von Mises stress (GPa), gid of the max\n", s->atoms->nGlobal, omega, samples);
   const double* last = NULL;
   for (int k = 0; k < samples; ++k) {
      last = rows + 8 * (size_t)k;
      fprintf(f, "%.0f %.17g %.17g %.17g %.17g %.17g %.0f\n", last[0], last[1] * eVperA3inGPa, last[2] * eVperA3inGPa, last[3] * eVperA3inGPa,
              last[4] * eVperA3inGPa, last[5] * eVperA3inGPa, last[6]);
   }
   fclose(f);
   if (pos && ten) {
      const StressDump dump = { ten, eVperA3inGPa / omega, s->stressDumpMin };
      char tail[256];
      snprintf(tail, sizeof tail, "stress:R:6:vm:R:1:gid:I:1 step=%d units=GPa atomicVolume=%.17g minVM=%.17g", iStep, omega, s->stressDumpMin);
      writeXyz(s->stressDump, s, pos, tail, stressXyzRow, &dump);
   }
   free(pos); free(ten);
   if (yaml) fprintf(yaml, "Stress:\n  Units: GPa\n  samples: %d\n  file: %s\n  finalMeanPressure: %.12e\n  finalMeanVonMises: %.12e\n  finalMaxVonMises: %.12e\n\n", samples, s->stressFile,
           last ? last[1] * eVperA3inGPa : 0.0, last ? last[4] * eVperA3inGPa : 0.0, last ? last[5] * eVperA3inGPa : 0.0);
}

/* --strain: the state at the end of global step strainRef becomes the reference */
static void startStrain(SimFlat* s)
{
   const int rc = comdStrainReference(s, 1);
   if (rc < 0) { printf("Error: --strain needs the device state.\n"); exit(-1); }
   if (rc > 0) { printf("Error: --strain: no device memory for the reference positions of %d atoms.\n", s->atoms->nGlobal); exit(-1); }
}

/* --strain: one more row {step, atoms, invalid atoms, mean / max shear strain, the gid of the max, mean volumetric strain, mean / max D^2min, atoms at or above
 * the threshold} from the device reduction */
static void sampleStrain(SimFlat* s, int iStep)
{
   double* row = (double*)nextRow(&s->strainRows, 10 * sizeof(double));
   row[0] = (double)iStep;
   if (comdStrainSummary(s, s->strainCutoff, s->strainThreshold, row + 1) != 0) { printf("Error: --strain needs the device state and a reference.\n"); exit(-1); }
   s->strainMaxShearNow = row[4];
}

static double shearOf(const double* e)
{
   const double d0 = e[0] - e[1], d1 = e[1] - e[2], d2 = e[2] - e[0];
   return sqrt(((e[3] * e[3] + e[4] * e[4]) + e[5] * e[5]) + ((d0 * d0 + d1 * d1) + d2 * d2) / 6.0);
}

/* --strain: the file: a header line, then the rows of sampleStrain.  --strainDump: the tensors of the last step as extended XYZ, Cu x y z exx eyy ezz eyz exz
 * exy shear vol d2min n gid, the atoms whose shear strain is at least --strainDumpMin (0: all atoms, the invalid ones with their NaNs included); the positions
 * gathered by gid over the ranks as the tensors are.  The YAML block names the file and gives the last sample. */
typedef struct { const double* ten; const int* cnt; double min; } StrainDump;      /* min 0: all atoms */
static int strainXyzRow(FILE* f, size_t g, const void* ctx)
{
   const StrainDump* d = (const StrainDump*)ctx;
   const double* t = d->ten + 7 * g;
   const double shear = shearOf(t);
   if (f) fprintf(f, " %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %zu\n", t[0], t[1], t[2], t[3], t[4], t[5], shear, ((t[0] + t[1]) + t[2]) / 3.0, t[6], d->cnt[g], g);
   return !(d->min > 0.0) || shear >= d->min;
}

static void writeStrain(FILE* yaml, SimFlat* s, int iStep)
{
   const size_t n = (size_t)s->atoms->nGlobal;
   double *pos = NULL, *ten = NULL;
   int* cnt = NULL;
   if (s->strainDump[0]) {          /* collective: before the other ranks leave */
      pos = positionsByGid(s);
      ten = (double*)malloc((n ? 7 * n : 1) * sizeof(double));
      cnt = (int*)malloc((n ? n : 1) * sizeof(int));
      if (comdAtomStrain(s, s->strainCutoff, ten, cnt) != 0) { printf("Error: --strainDump needs the device state and a reference.\n"); exit(-1); }
   }
   if (!printRank()) { free(pos); free(ten); free(cnt); return; }
   const int samples = s->strainRows.n;
   const double* rows = (const double*)s->strainRows.rows;
   FILE* f = openReport(s->strainFile);
   fprintf(f, "# Strain: N %d L0 %.17g %.17g %.17g reference step %d cutoff %.17g A threshold %.17g samples %d | columns: step, mean / max shear strain, "
              "gid of the max, mean volumetric strain, mean / max D2min (A^2), atoms at or above the threshold, invalid atoms\n",
           s->atoms->nGlobal, s->strainL0[0], s->strainL0[1], s->strainL0[2], s->strainRef, s->strainCutoff, s->strainThreshold, samples);
   const double* last = NULL;
   for (int k = 0; k < samples; ++k) {
      last = rows + 10 * (size_t)k;
      fprintf(f, "%.0f %.17g %.17g %.0f %.17g %.17g %.17g %.0f %.0f\n", last[0], last[3], last[4], last[5], last[6], last[7], last[8], last[9], last[2]);
   }
   fclose(f);
   if (pos && ten) {
      const StrainDump dump = { ten, cnt, s->strainDumpMin };
      char tail[256];
      snprintf(tail, sizeof tail, "strain:R:6:shear:R:1:vol:R:1:d2min:R:1:n:I:1:gid:I:1 step=%d referenceStep=%d cutoff=%.17g minShear=%.17g",
               iStep, s->strainRef, s->strainCutoff, s->strainDumpMin);
      writeXyz(s->strainDump, s, pos, tail, strainXyzRow, &dump);
   }
   free(pos); free(ten); free(cnt);
   if (!yaml) return;
   static const double none[10] = { 0.0 };
   if (!last) last = none;
   fprintf(yaml, "Strain:\n  referenceStep: %d\n  cutoff: %.12e\n  threshold: %.12e\n  samples: %d\n  file: %s\n", s->strainRef, s->strainCutoff, s->strainThreshold, samples, s->strainFile);
   fprintf(yaml, "  finalMeanShear: %.12e\n  finalMaxShear: %.12e\n  finalMeanVolumetric: %.12e\n  finalMeanD2min: %.12e\n  finalMaxD2min: %.12e\n", last[3], last[4], last[6], last[7], last[8]);
   fprintf(yaml, "  finalAboveThreshold: %.0f\n  finalInvalid: %.0f\n\n", last[9], last[2]);
}

/* --heatflux: one more row {step, time, the nine sums of comdHeatFlux, temperature, volume}.  Only at a printed step are the per-atom energies those of the
 * current positions: timestep() asks the force kernels for them on its last step alone */
static void sampleHeatFlux(SimFlat* s, int iStep)
{
   double* row = (double*)nextRow(&s->hfRows, 13 * sizeof(double));
   row[0] = (double)iStep; row[1] = iStep * s->dt;
   if (comdHeatFlux(s, row + 2) != 0) { printf("Error: --heatflux needs the device state.\n"); exit(-1); }
   row[11] = (s->eKinetic / s->atoms->nGlobal) / (kB_eV * 1.5);
   row[12] = (double)s->domain->globalExtent[0] * s->domain->globalExtent[1] * s->domain->globalExtent[2];
   s->hfJxNow = ((row[2] + row[5]) + row[8]) / row[12];
}

#define eVperFsAKinWperMK 1.602176634e6      /* 1 eV/(fs A K) in W/(m K) */

/* --heatflux: the two files and the YAML block.  hfFile: a header with N, V, the time between samples, the start step and the number of samples, then per
 * sample the step, the time, J V = jk + jp + jv, its convective part jk + jp and its virial part jv (eV A/fs).  hfAcfFile: per lag k < M the time k dt, the
 * autocorrelation C_x, C_y, C_z of J V (comdHeatFluxAcf) and the running conductivity kappa(k) = dt trapezoid_0^k (C_x + C_y + C_z) / (3 V kB T^2) in W/(m K),
 * with T and V the means over the samples (V: the box may strain). */
static void writeHeatFlux(FILE* yaml, SimFlat* s, int iStep)
{
   if (!printRank()) return;
   const int samples = s->hfRows.n;
   const double* rows = (const double*)s->hfRows.rows;
   const double dtSample = (double)s->printRate * s->dt;
   double meanT = 0.0, meanV = 0.0, meanJ[3] = { 0.0, 0.0, 0.0 };
   double* jv = (double*)malloc((samples ? 3 * (size_t)samples : 1) * sizeof(double));
   for (int k = 0; k < samples; ++k) {
      const double* r = rows + 13 * (size_t)k;
      for (int a = 0; a < 3; ++a) { jv[3 * (size_t)k + a] = (r[2 + a] + r[5 + a]) + r[8 + a]; meanJ[a] += jv[3 * (size_t)k + a]; }
      meanT += r[11]; meanV += r[12];
   }
   if (samples) { meanT /= samples; meanV /= samples; for (int a = 0; a < 3; ++a) meanJ[a] /= samples; }
   else meanV = (double)s->domain->globalExtent[0] * s->domain->globalExtent[1] * s->domain->globalExtent[2];
   FILE* f = openReport(s->hfFile);
   fprintf(f, "# HeatFlux: N %d V %.17g A^3 (mean of the samples) dt %.17g fs between samples startStep %d samples %d | columns: step, time (fs), "
              "J V x y z (eV A/fs), convective part x y z, virial part x y z\n", s->atoms->nGlobal, meanV, dtSample, s->hfStart, samples);
   for (int k = 0; k < samples; ++k) {
      const double* r = rows + 13 * (size_t)k;
      fprintf(f, "%.0f %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", r[0], r[1], jv[3 * (size_t)k], jv[3 * (size_t)k + 1], jv[3 * (size_t)k + 2],
              r[2] + r[5], r[3] + r[6], r[4] + r[7], r[8], r[9], r[10]);
   }
   fclose(f);
   int window = s->hfWindow > 0 ? s->hfWindow : samples / 2;
   const int clipped = window > samples;
   if (clipped) window = samples;
   if (window < 1) window = samples > 0 ? 1 : 0;
   double* acf = (double*)malloc((3 * (size_t)window + 1) * sizeof(double));
   if (window > 0) comdHeatFluxAcf(jv, samples, window, acf);
   f = openReport(s->hfAcfFile);
   fprintf(f, "# HeatFluxACF: N %d V %.17g A^3 T %.17g K (means of the samples) dt %.17g fs samples %d window %d%s | columns: lag time (fs), "
              "C x y z of J V (eV^2 A^2/fs^2), running kappa (W/m/K)\n", s->atoms->nGlobal, meanV, meanT, dtSample, samples, window,
           clipped ? " (clipped to the samples)" : "");
   const double unit = meanT > 0.0 ? eVperFsAKinWperMK / (3.0 * meanV * kB_eV * meanT * meanT) : 0.0;
   double integral = 0.0, kappa = 0.0;
   for (int k = 0; k < window; ++k) {
      const double* c = acf + 3 * (size_t)k;
      if (k > 0) integral += 0.5 * (((c[-3] + c[-2]) + c[-1]) + ((c[0] + c[1]) + c[2])) * dtSample;
      kappa = unit * integral;
      fprintf(f, "%.17g %.17g %.17g %.17g %.17g\n", k * dtSample, c[0], c[1], c[2], kappa);
   }
   fclose(f);
   free(acf); free(jv);
   if (!yaml) return;
   fprintf(yaml, "HeatFlux:\n  startStep: %d\n  samples: %d\n  window: %d\n  file: %s\n  acfFile: %s\n", s->hfStart, samples, window, s->hfFile, s->hfAcfFile);
   fprintf(yaml, "  meanJV: [ %.12e, %.12e, %.12e ]\n  fluxUnits: eV A/fs\n", meanJ[0], meanJ[1], meanJ[2]);
   if (samples >= 2) fprintf(yaml, "  kappa: %.12e\n", kappa); else fprintf(yaml, "  kappa: n/a\n");
   fprintf(yaml, "  kappaUnits: W/m/K\n\n");
}

/* --sk: the amplitudes of this printed step go through the powder average into the sums; the Bragg order is a call of its own (M = 1 at the strides of the cells) */
static void sampleSk(SimFlat* s, int iStep)
{
   const int M = s->sk, W = 2 * M + 1, n = s->skBins;
   double* rho = (double*)malloc((size_t)2 * (M + 1) * W * W * sizeof(double));
   double* now = (double*)malloc(3 * (size_t)n * sizeof(double));
   const double box[3] = { (double)s->domain->globalExtent[0], (double)s->domain->globalExtent[1], (double)s->domain->globalExtent[2] };
   if (comdStructureFactor(s, M, s->skStride, rho) != 0 || comdBraggOrder(s, &s->skBraggNow) != 0) { printf("Error: --sk needs the device state.\n"); exit(-1); }
   if (comdStructureFactorRadial(rho, M, s->skStride, box, n, now, now + n, now + 2 * n) != 0) { printf("Error: --sk: the powder average was refused.\n"); exit(-1); }
   for (int b = 0; b < n; ++b) if (now[2 * n + b] > 0.0) { s->skSum[b] += now[n + b] * now[2 * n + b]; s->skSum[n + b] += now[2 * n + b]; }
   free(rho); free(now);
   if (s->skSamples == 0) s->skBraggFirst = s->skBraggNow;
   s->skBraggSum += s->skBraggNow;
   for (int a = 0; a < 3; ++a) s->skBoxSum[a] += box[a];
   s->skSamples++;
   (void)iStep;
}

/* --sk: the file and the YAML block.  skFile: a header with N, M, the strides, the bins, the samples and the mean box, then per bin the |k| centre (1/A) on the mean
 * box, S averaged over the samples and the vectors of the bin, and the vectors per sample (h > 0 twice); an empty bin prints nan */
static void writeSk(FILE* yaml, SimFlat* s, int iStep)
{
   if (!printRank()) return;
   const int M = s->sk, n = s->skBins, samples = s->skSamples;
   double box[3], kMax = INFINITY;
   for (int a = 0; a < 3; ++a) {
      box[a] = samples ? s->skBoxSum[a] / samples : (double)s->domain->globalExtent[a];
      const double k = (6.283185307179586 * (double)(s->skStride[a] * M)) / box[a];
      if (k < kMax) kMax = k;
   }
   const double dk = kMax / n;
   FILE* f = openReport(s->skFile);
   fprintf(f, "# StructureFactor: N %d M %d stride %d %d %d bins %d samples %d startStep %d meanL %.17g %.17g %.17g A | columns: |k| centre (1/A), S averaged over "
              "samples and vectors, vectors per sample\n", s->atoms->nGlobal, M, s->skStride[0], s->skStride[1], s->skStride[2], n, samples, s->skStart, box[0], box[1], box[2]);
   int best = -1;
   for (int b = 0; b < n; ++b) {
      const double count = s->skSum[n + b];
      if (count > 0.0) {
         const double mean = s->skSum[b] / count;
         if (best < 0 || mean > s->skSum[best] / s->skSum[n + best]) best = b;
         fprintf(f, "%.17g %.17g %.17g\n", (b + 0.5) * dk, mean, count / samples);
      } else fprintf(f, "%.17g nan %.17g\n", (b + 0.5) * dk, 0.0);
   }
   fclose(f);
   if (!yaml) return;
   fprintf(yaml, "StructureFactor:\n  kMaxIndex: %d\n  stride: [ %d, %d, %d ]\n  bins: %d\n  samples: %d\n  file: %s\n", M, s->skStride[0], s->skStride[1], s->skStride[2], n, samples, s->skFile);
   if (best >= 0) fprintf(yaml, "  kOfHighestS: %.12e\n", (best + 0.5) * dk); else fprintf(yaml, "  kOfHighestS: n/a\n");
   if (samples) fprintf(yaml, "  braggFirst: %.12e\n  braggFinal: %.12e\n  braggMean: %.12e\n\n", s->skBraggFirst, s->skBraggNow, s->skBraggSum / samples);
   else fprintf(yaml, "  braggFirst: n/a\n  braggFinal: n/a\n  braggMean: n/a\n\n");
   (void)iStep;
}

/* --steinhardt: one more row {step, valid atoms, invalid atoms, mean q4, mean q6, min q6, the gid of the min, max q6, mean w4, mean w6, atoms at or above the
 * threshold} from the device reduction */
static void sampleSteinhardt(SimFlat* s, int iStep)
{
   double* row = (double*)nextRow(&s->stRows, 11 * sizeof(double));
   row[0] = (double)iStep;
   if (comdSteinhardtSummary(s, s->stSolid, row + 1) != 0) { printf("Error: --steinhardt needs the device state.\n"); exit(-1); }
   s->stMeanQ6Now = row[4];
}

/* --steinhardt: the file: a header line, then the rows of sampleSteinhardt.  --stDump: the values of the last step as extended XYZ, Cu x y z q4 q6 w4 w6 gid, the
 * atoms whose q6 is at most --stDumpMax (+inf: all atoms) and the invalid ones with their NaNs; the positions gathered by gid over the ranks as the values
 * are.  The YAML block names the file and gives the last sample's mean q6 and the fraction of the atoms at or above the threshold. */
typedef struct { const double* q; double max; } SteinhardtDump;
static int steinhardtXyzRow(FILE* f, size_t g, const void* ctx)
{
   const SteinhardtDump* d = (const SteinhardtDump*)ctx;
   const double* t = d->q + 4 * g;
   if (f) fprintf(f, " %.17g %.17g %.17g %.17g %zu\n", t[0], t[1], t[2], t[3], g);
   return !(t[1] > d->max);          /* a NaN stays in */
}

static void writeSteinhardt(FILE* yaml, SimFlat* s, int iStep)
{
   const size_t n = (size_t)s->atoms->nGlobal;
   double *pos = NULL, *q = NULL;
   if (s->stDump[0]) {          /* collective: before the other ranks leave */
      pos = positionsByGid(s);
      q = (double*)malloc((n ? 4 * n : 1) * sizeof(double));
      if (comdSteinhardt(s, q) != 0) { printf("Error: --stDump needs the device state.\n"); exit(-1); }
   }
   if (!printRank()) { free(pos); free(q); return; }
   const int samples = s->stRows.n;
   const double* rows = (const double*)s->stRows.rows;
   FILE* f = openReport(s->stFile);
   fprintf(f, "# Steinhardt: N %d threshold %.17g samples %d | columns: step, valid atoms, invalid atoms (fewer than 12 neighbours), mean q4, mean q6, min q6, "
              "gid of the min, max q6, mean w4, mean w6, atoms with q6 >= threshold\n", s->atoms->nGlobal, s->stSolid, samples);
   const double* last = NULL;
   for (int k = 0; k < samples; ++k) {
      last = rows + 11 * (size_t)k;
      fprintf(f, "%.0f %.0f %.0f %.17g %.17g %.17g %.0f %.17g %.17g %.17g %.0f\n", last[0], last[1], last[2], last[3], last[4], last[5], last[6], last[7], last[8], last[9], last[10]);
   }
   fclose(f);
   if (pos && q) {
      const SteinhardtDump dump = { q, s->stDumpMax };
      char tail[256];
      snprintf(tail, sizeof tail, "q4:R:1:q6:R:1:w4:R:1:w6:R:1:gid:I:1 step=%d maxQ6=%.17g", iStep, s->stDumpMax);
      writeXyz(s->stDump, s, pos, tail, steinhardtXyzRow, &dump);
   }
   free(pos); free(q);
   if (!yaml) return;
   const double atoms = last ? last[1] + last[2] : 0.0;
   fprintf(yaml, "Steinhardt:\n  threshold: %.12e\n  samples: %d\n  file: %s\n  finalMeanQ6: %.12e\n  finalSolidFraction: %.12e\n\n", s->stSolid, samples, s->stFile,
           last ? last[4] : 0.0, atoms > 0.0 ? last[10] / atoms : 0.0);
}

/* --elastic: one more row {step, T (K), V (A^3), the pair stress sigma_I = -W_I / V (6) and the upper triangle of B / V (21), eV/A^3} from the tensors computePressure
 * has just left in W, V and the device's Born matrix */
#define ELASTIC_ROW 30
#define ELASTIC_T_REST 1e-9            /* K: below this mean temperature the lattice is at rest (a -T 0 run picks up 1e-28 K from forces that are rounding errors, and
                                        * V / kB T times the rounding noise of the stress is no fluctuation term): T counts as 0 */
static void sampleElastic(SimFlat* s, int iStep)
{
   double* row = (double*)nextRow(&s->elRows, ELASTIC_ROW * sizeof(double));
   double born[21];
   if (comdBornMatrix(s, born) != 0) { printf("Error: --elastic needs the device state.\n"); exit(-1); }
   row[0] = (double)iStep;
   row[1] = (s->eKinetic / s->atoms->nGlobal) / (kB_eV * 1.5);
   row[2] = (double)s->V;
   for (int c = 0; c < 6; ++c) row[3 + c] = -(double)s->W[c] / s->V;
   for (int c = 0; c < 21; ++c) row[9 + c] = born[c] / s->V;
   s->elC11BornNow = (row[9] + row[15] + row[20]) / 3.0;
}

/* the cubic averages of a 6 x 6 matrix: (11 + 22 + 33) / 3, (12 + 13 + 23) / 3, (44 + 55 + 66) / 3 */
static void cubicAverages(const double* m, double out[3])
{
   out[0] = (m[0] + m[7] + m[14]) / 3.0; out[1] = (m[1] + m[2] + m[8]) / 3.0; out[2] = (m[21] + m[28] + m[35]) / 3.0;
}

/* --elastic: the file: a header line, per sample the step, T, V, the six pair stresses and the 21 B_IJ / V in GPa, then the 6 x 6 C in GPa behind '#'.  The
 * YAML block gives C11, C12, C44 (cubic averages) with their Born, fluctuation and kinetic parts, K = (C11 + 2 C12) / 3, G_V = (C11 - C12 + 3 C44) / 5,
 * A = 2 C44 / (C11 - C12) and the Cauchy pressure C12 - C44; T and V are the means over the samples, a T below ELASTIC_T_REST counting as 0.  Derivatives with respect to the Lagrangian strain:
 * under stress they differ from stress-strain coefficients by terms in the stress. */
static void writeElastic(FILE* yaml, SimFlat* s, int iStep)
{
   if (!printRank()) return;
   const int samples = s->elRows.n;
   const double* rows = (const double*)s->elRows.rows;
   double T = 0.0, V = 0.0;
   for (int k = 0; k < samples; ++k) { T += rows[ELASTIC_ROW * (size_t)k + 1] / samples; V += rows[ELASTIC_ROW * (size_t)k + 2] / samples; }
   if (T < ELASTIC_T_REST) T = 0.0;
   const size_t nRows = samples > 0 ? (size_t)samples : 1;
   double *born = (double*)malloc(nRows * 21 * sizeof(double)), *stress = (double*)malloc(nRows * 6 * sizeof(double));
   for (int k = 0; k < samples; ++k) {
      for (int c = 0; c < 6; ++c) stress[6 * (size_t)k + c] = rows[ELASTIC_ROW * (size_t)k + 3 + c];
      for (int c = 0; c < 21; ++c) born[21 * (size_t)k + c] = rows[ELASTIC_ROW * (size_t)k + 9 + c];
   }
   double part[3][36], C[36];
   memset(part, 0, sizeof part);
   if (samples > 0) comdElasticConstants(born, stress, samples, V, T, (double)s->atoms->nGlobal, part[0], part[1], part[2]);
   for (int c = 0; c < 36; ++c) C[c] = (part[0][c] + part[1][c]) + part[2][c];
   free(born); free(stress);
   FILE* f = openReport(s->elFile);
   fprintf(f, "# Elastic: N %d samples %d T %.17g V %.17g | columns: step, T (K), V (A^3), pair stress xx yy zz yz xz xy (GPa, tension positive), "
              "B/V 11 12 13 14 15 16 22 23 24 25 26 33 34 35 36 44 45 46 55 56 66 (GPa)\n", s->atoms->nGlobal, samples, T, V);
   for (int k = 0; k < samples; ++k) {
      const double* r = rows + ELASTIC_ROW * (size_t)k;
      fprintf(f, "%.0f %.17g %.17g", r[0], r[1], r[2]);
      for (int c = 3; c < ELASTIC_ROW; ++c) fprintf(f, " %.17g", r[c] * eVperA3inGPa);
      fprintf(f, "\n");
   }
   fprintf(f, "# C (GPa) = <B>/V - V/(kB T) (<s s> - <s><s>) + N kB T/V kappa, Voigt order xx yy zz yz xz xy:\n");
   for (int i = 0; i < 6; ++i) {
      fprintf(f, "#");
      for (int j = 0; j < 6; ++j) fprintf(f, " %.17g", C[6 * i + j] * eVperA3inGPa);
      fprintf(f, "\n");
   }
   fclose(f);
   if (!yaml) return;
   static const char* name[3] = { "C11", "C12", "C44" };
   double c[3], b[3], fl[3], kin[3];
   cubicAverages(C, c); cubicAverages(part[0], b); cubicAverages(part[1], fl); cubicAverages(part[2], kin);
   fprintf(yaml, "Elastic:\n  samples: %d\n  fromStep: %d\n  temperature: %.12e\n  volume: %.12e\n  file: %s\n  Units: GPa\n", samples, s->elStart, T, V, s->elFile);
   for (int m = 0; m < 3; ++m)
      fprintf(yaml, "  %s: %.12e\n  %sBorn: %.12e\n  %sFluctuation: %.12e\n  %sKinetic: %.12e\n", name[m], c[m] * eVperA3inGPa, name[m], b[m] * eVperA3inGPa,
              name[m], fl[m] * eVperA3inGPa, name[m], kin[m] * eVperA3inGPa);
   fprintf(yaml, "  bulkModulus: %.12e\n  shearModulusVoigt: %.12e\n  cauchyPressure: %.12e\n", (c[0] + 2.0 * c[1]) / 3.0 * eVperA3inGPa,
           (c[0] - c[1] + 3.0 * c[2]) / 5.0 * eVperA3inGPa, (c[1] - c[2]) * eVperA3inGPa);
   if (c[0] != c[1]) fprintf(yaml, "  anisotropy: %.12e\n\n", 2.0 * c[2] / (c[0] - c[1])); else fprintf(yaml, "  anisotropy: n/a\n\n");
   (void)iStep;
}

/* ---- the table: one row per report, in the order of the columns of printThings and of the YAML blocks ---------------------------------------------------------
 * on      the row applies to this run;
 * from    the first global step it samples at (NULL: 0), start what is done when the run reaches that step: at a printed step under the report's timer, just
 *         before the sample; between two printed steps comdMain splits the interval there, and it runs under the timestep timer;
 * sample  at every printed step >= from, under timer (NO_TIMER: under none);
 * header, column   its part of the header line of printThings and of every row;
 * write   the files and the YAML block at the end of the run, under the same timer when writeTimed.
 * A report whose parts do not share one condition has a row per condition. */
#define NO_TIMER numberOfTimers
typedef struct ReportSt {
   int  (*on)(const SimFlat* s);
   int  (*from)(const SimFlat* s);
   void (*start)(SimFlat* s);
   void (*sample)(SimFlat* s, int iStep);
   enum TimerHandle timer;
   const char* header;
   void (*column)(const SimFlat* s);
   void (*write)(FILE* yaml, SimFlat* s, int iStep);
   int  writeTimed;
} Report;

static int virialOn(const SimFlat* s)      { return s->pressure || s->deformReport || s->baroReport || s->elastic; }
static int pressureShown(const SimFlat* s) { return s->pressure || s->baroReport; }
static int pressureOn(const SimFlat* s)    { return s->pressure; }
static int rdfOn(const SimFlat* s)         { return s->rdfBins; }
static int msdOn(const SimFlat* s)         { return s->msd; }
static int cspOn(const SimFlat* s)         { return s->csp; }
static int cnaOn(const SimFlat* s)         { return s->cna; }
static int deformOn(const SimFlat* s)      { return s->deformReport; }
static int baroOn(const SimFlat* s)        { return s->baroReport; }
static int baroVolumeShown(const SimFlat* s) { return s->baroReport && !s->deformReport; }      /* beside --erate the column is there already */
static int stressOn(const SimFlat* s)      { return s->stress; }
static int strainOn(const SimFlat* s)      { return s->strain; }
static int heatfluxOn(const SimFlat* s)    { return s->heatflux; }
static int profileOn(const SimFlat* s)     { return s->profile; }
static int mpOn(const SimFlat* s)          { return s->mpReport; }
static int skOn(const SimFlat* s)          { return s->sk; }
static int steinhardtOn(const SimFlat* s)  { return s->steinhardt; }
static int elasticOn(const SimFlat* s)     { return s->elastic; }

static int msdFrom(const SimFlat* s)       { return s->msdStart; }
static int strainFrom(const SimFlat* s)    { return s->strainRef; }
static int heatfluxFrom(const SimFlat* s)  { return s->hfStart; }
static int profileFrom(const SimFlat* s)   { return s->profStart; }
static int skFrom(const SimFlat* s)        { return s->skStart; }
static int elasticFrom(const SimFlat* s)   { return s->elStart; }

static double volumeRatio(const SimFlat* s) { return (double)s->V / (s->box0[0] * s->box0[1] * s->box0[2]); }
static void pressureColumn(const SimFlat* s) { fprintf(screenOut, " %16.10f", pressureOf(s) * eVperA3inGPa); }
static void msdColumn(const SimFlat* s)      { fprintf(screenOut, " %16.10e", s->msdNow); }
static void cspColumn(const SimFlat* s)      { fprintf(screenOut, " %12d", s->cspDefectsNow); }
static void cnaColumn(const SimFlat* s)      { fprintf(screenOut, " %12lld", s->cnaNonFccNow); }
static void deformColumns(const SimFlat* s)  { fprintf(screenOut, " %14.10f %16.10f", volumeRatio(s), -((double)s->K[0] + s->W[0]) / s->V * eVperA3inGPa); }
static void volumeColumn(const SimFlat* s)   { fprintf(screenOut, " %14.10f", volumeRatio(s)); }
static void stressColumn(const SimFlat* s)   { fprintf(screenOut, " %16.10f", s->stressMaxVmNow * eVperA3inGPa); }
static void strainColumn(const SimFlat* s)   { fprintf(screenOut, " %16.10f", s->strainMaxShearNow); }
static void heatfluxColumn(const SimFlat* s) { fprintf(screenOut, " %19.10e", s->hfJxNow); }
static void mpColumn(const SimFlat* s)       { fprintf(screenOut, " %19.10e", s->mpExchanged); }
static void skColumn(const SimFlat* s)       { fprintf(screenOut, " %16.10f", s->skBraggNow); }
static void steinhardtColumn(const SimFlat* s) { fprintf(screenOut, " %16.10f", s->stMeanQ6Now); }
static void elasticColumn(const SimFlat* s)  { fprintf(screenOut, " %16.10f", s->elC11BornNow * eVperA3inGPa); }

static const Report reports[] = {
   { .on = virialOn,        .sample = samplePressure, .timer = pressureTimer },      /* first: the samplers below read W, K, V */
   { .on = pressureShown,   .header = "    Pressure(GPa)", .column = pressureColumn },
   { .on = pressureOn,      .write = writePressure },
   { .on = rdfOn,           .sample = sampleRdf, .timer = rdfTimer, .write = writeRdf },
   { .on = msdOn,           .from = msdFrom, .start = startMsd, .sample = sampleMsd, .timer = msdTimer, .header = "         MSD(A^2)", .column = msdColumn, .write = writeMsd },
   { .on = cspOn,           .sample = sampleCsp, .timer = cspTimer, .header = "      Defects", .column = cspColumn, .write = writeCsp },
   { .on = cnaOn,           .sample = sampleCna, .timer = cnaTimer, .header = "       NonFCC", .column = cnaColumn, .write = writeCna },
   { .on = deformOn,        .sample = sampleDeform, .timer = NO_TIMER, .header = "           V/V0         Sxx(GPa)", .column = deformColumns, .write = writeDeform },
   { .on = baroOn,          .write = writeBaro },      /* its rows: baroCouple, inside timestep() */
   { .on = baroVolumeShown, .header = "           V/V0", .column = volumeColumn },
   { .on = stressOn,        .sample = sampleStress, .timer = stressTimer, .header = "       MaxVM(GPa)", .column = stressColumn, .write = writeStress, .writeTimed = 1 },
   { .on = strainOn,        .from = strainFrom, .start = startStrain, .sample = sampleStrain, .timer = strainTimer, .header = "         MaxShear", .column = strainColumn,
     .write = writeStrain, .writeTimed = 1 },
   { .on = heatfluxOn,      .from = heatfluxFrom, .sample = sampleHeatFlux, .timer = heatfluxTimer, .header = "       Jx(eV/A^2/fs)", .column = heatfluxColumn,
     .write = writeHeatFlux, .writeTimed = 1 },
   { .on = profileOn,       .from = profileFrom, .sample = sampleProfile, .timer = profileTimer, .write = writeProfile, .writeTimed = 1 },      /* and the files and the block of --mp */
   { .on = mpOn,            .header = "              dE(eV)", .column = mpColumn },      /* its rows: mpExchange, inside timestep() */
   { .on = skOn,            .from = skFrom, .sample = sampleSk, .timer = skTimer, .header = "           S111/N", .column = skColumn, .write = writeSk },
   { .on = steinhardtOn,    .sample = sampleSteinhardt, .timer = steinhardtTimer, .header = "           MeanQ6", .column = steinhardtColumn, .write = writeSteinhardt },
   { .on = elasticOn,       .from = elasticFrom, .sample = sampleElastic, .timer = elasticTimer, .header = "        C11B(GPa)", .column = elasticColumn, .write = writeElastic },
};
#define FOR_REPORTS(r, s) for (const Report* r = reports; r < reports + sizeof reports / sizeof reports[0]; ++r) if (r->on(s))

static int fromOf(const Report* r, const SimFlat* s) { return r->from ? r->from(s) : 0; }

void reportsSample(SimFlat* s, int iStep)
{
   FOR_REPORTS(r, s) if (r->sample && iStep >= fromOf(r, s)) {
      if (r->timer != NO_TIMER) startTimer(r->timer);
      if (r->start && iStep == fromOf(r, s)) r->start(s);
      r->sample(s, iStep);
      if (r->timer != NO_TIMER) stopTimer(r->timer);
   }
}

/* the first step in (iStep, end) at which a report starts, end when there is none; reportsStart: what starts at iStep does */
int reportsNextStart(const SimFlat* s, int iStep, int end)
{
   FOR_REPORTS(r, s) if (r->start && fromOf(r, s) > iStep && fromOf(r, s) < end) end = fromOf(r, s);
   return end;
}

void reportsStart(SimFlat* s, int iStep)
{
   FOR_REPORTS(r, s) if (r->start && fromOf(r, s) == iStep) r->start(s);
}

/* printThings: the report columns of the header line (header != 0) or of a row */
void reportsColumns(const SimFlat* s, int header)
{
   FOR_REPORTS(r, s) if (r->column) { if (header) fprintf(screenOut, "%s", r->header); else r->column(s); }
}

void reportsWrite(FILE* yaml, SimFlat* s, int iStep)
{
   FOR_REPORTS(r, s) if (r->write) {
      if (r->writeTimed) startTimer(r->timer);
      r->write(yaml, s, iStep);
      if (yaml) fflush(yaml);
      if (r->writeTimed) stopTimer(r->timer);
   }
}

void reportsFree(SimFlat* s)
{
   RowTable* tables[] = { &s->msdRows, &s->cspRows, &s->cnaRows, &s->deformRows, &s->baroRows, &s->mpRows, &s->stressRows, &s->strainRows, &s->hfRows, &s->stRows, &s->elRows };
   for (size_t i = 0; i < sizeof tables / sizeof tables[0]; ++i) free(tables[i]->rows);
   free(s->rdfSum); free(s->cspLast); free(s->cnaLast); free(s->profSum); free(s->skSum);
}
