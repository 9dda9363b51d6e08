// comd_device.hip -- launch wrappers and device-memory management behind include/comd_hip.h.
//
// Stands where the reference's gpu_kernels.cu (extern "C" wrappers, :69-660, :1013-1059) and the device half of
// gpu_utility.c (:32-347, :432-653) do.  gfx950 only; built with hipcc --offload-arch=gfx950.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <map>
#include <utility>

#include "comd_hip.h"
#include "device_common.h"
#include "lj_kernels.h"
#include "lj_table_kernels.h"
#include "eam_kernels.h"
#include "step_kernels.h"
#include "nl_kernels.h"
#include "eam_brick_kernels.h"
#include "eam_atom_brick_kernels.h"
#include "virial_kernels.h"
#include "fdotr_kernels.h"
#include "profile_kernels.h"
#include "mp_kernels.h"
#include "sk_kernels.h"
#include "rdf_kernels.h"
#include "csp_kernels.h"
#include "cna_kernels.h"
#include "stress_kernels.h"
#include "strain_kernels.h"
#include "steinhardt_kernels.h"
#include "born_kernels.h"
#include "heatflux_kernels.h"
#include "langevin_kernels.h"
#include "msd_kernels.h"
#include "deform_kernels.h"

static int g_rank = 0;

#define HIP_CHECK(cmd)                                                                                     \
   do {                                                                                                    \
      hipError_t status_ = (cmd);                                                                          \
      if (status_ != hipSuccess) {                                                                         \
         int dev_ = -1; (void)hipGetDevice(&dev_);                                                         \
         fprintf(stderr, "Rank %d, GPU: %d, Error in file %s at line %d\n", g_rank, dev_, __FILE__, __LINE__); \
         fprintf(stderr, "HIP error %d: %s\n", (int)status_, hipGetErrorString(status_));                  \
         exit(-1);                                                                                         \
      }                                                                                                    \
   } while (0)

#define LAUNCH_CHECK() HIP_CHECK(hipGetLastError())

static inline hipStream_t S(comdStream_t s) { return (hipStream_t)s; }
static inline int ceilDiv(long a, long b) { return (int)((a + b - 1) / b); }

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (device, kernel): remember the largest size asked for per pair
static void allowDynamicLds(const void* fn, size_t lds)
{
   static std::map<std::pair<int, const void*>, size_t> granted;
   int dev = 0; HIP_CHECK(hipGetDevice(&dev));
   size_t& g = granted[std::make_pair(dev, fn)];
   if (lds > g) { HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); g = lds; }
}

// ---- tuning: the COMD_* environment variables of this file, read once per simulation ---------------------------------------
// A variable changed after AllocateGpu no longer reaches that simulation.  All are optional, for tests, A/B runs and diagnosis (README.md has the same table).
struct ComdTuning {
   //                             variable                      meaning                                                                                  default
   bool   nlGlobal;            // COMD_NL_GLOBAL (set)          Verlet lists in the plain 32-bit global-slot format, not the LDS-relative 16-bit ones      off
   bool   eamNlLds;            // COMD_EAM_NL=lds               round 3's EAM list kernel (a wave stages every cell's stencil), not rows of the brick kernel  off
   int    ljWaves;             // COMD_LJ_WAVES=k (> 0)         at most k waves per cell in LJ_Force_thread_atom (tests: the extra-chunk path)              cap/64
   bool   ljPrune;             // COMD_LJ_PRUNE=0               LJ thread_atom walks all 27 cells, no candidate lists                                       lists
   bool   ljPrefetch;          // COMD_LJ_PREFETCH=0            LJ thread_atom reads its candidate lists without the vector-side L2 prefetch (A/B runs)     prefetch
   int    ljListCap;           // COMD_LJ_LIST_CAP=n (> 0)      candidate rows of n entries, rounded up to 8 (tests: rows too short fall back to the walk)  70 % of a stencil
   double ljListBudgetMb;      // COMD_LJ_LIST_BUDGET_MB=x      memory the LJ candidate lists may take (tests: the fallback to the plain walk)              what is free
   bool   ljCtaSlabs;          // COMD_LJ_CTA_SLABS=1           LJ cta_cell in its slab form                                                                box-pruned form
   bool   eamCtaCell;          // COMD_EAM_CTA=cell             round 2's EAM cta_cell kernel (a wave stages every cell's stencil itself)                   brick kernel
   bool   eamThreadAtomCell;   // COMD_EAM_THREAD_ATOM=cell     round 2's EAM thread_atom kernel, not the thread-per-atom kernel on the brick image         brick image
   bool   eamGroups;           // COMD_EAM_GROUPS=0             the overlap mode's boundary / interior launches take the host's lists cell by cell          whole bricks
   int    eamBrickBy, eamBrickBz;      // COMD_EAM_BRICK=by,bz  cells of a brick of cta_cell and the list method (each >= 1, by * bz <= 64, block staged)   4,2
   int    eamImage;            // COMD_EAM_IMAGE=n (>= 64)      records of the brick's LDS image, rounded up to 8 (tests: bricks that outgrow it)           fullest block
   int    eamAblate;           // COMD_EAM_ABLATE=bits          EamBrickArgs.debug: parts of the brick kernels switched off (profiling; wrong results)      0
   bool   eamClamp;            // COMD_EAM_CLAMP=1              the brick kernels keep the table clamps of interpolate() where no pair needs them           dropped
   int    eamAtomRows;         // COMD_EAM_ATOM_ROWS=n (8..128) bytes of a thread's row in thread_atom, rounded down to 8 (tests: rows that overflow)       sphere + 50 %
   bool   eamAtomHandover;     // COMD_EAM_ATOM_HANDOVER=0      pass 3 of thread_atom tests again, reads no rows of pass 1                                  hand-over
   int    eamAtomBrickBy, eamAtomBrickBz;      // COMD_EAM_ATOM_BRICK=by,bz      cells of a thread_atom brick (as COMD_EAM_BRICK)                          first fit of 4,4 ...
   int    eamAtomLdsPad;       // COMD_EAM_ATOM_LDS_PAD=n       bytes of LDS a thread_atom launch asks for beyond its need (fewer workgroups per CU)        0
   int    eamCtaWaves;         // COMD_EAM_CTA_WAVES=k (1..8)   waves per workgroup of COMD_EAM_CTA=cell                                                    4
   int    eamStencil;          // COMD_EAM_STENCIL=n (>= 64)    records of the LDS slice of COMD_EAM_CTA=cell, rounded up to 8                              density + 20-30 %
   bool   nlSync;              // COMD_NL_SYNC=1                the deferred "rebuild the lists?" test (COMD_NL_DEFERRED) blocks every step                 off
   bool   eamListsEveryBuild;  // COMD_EAM_LISTS_EVERY_BUILD (set)  the brick lists of the EAM list method remade at every list build                      kept while they fit
   bool   nlBankOrder;         // COMD_NL_BANK_ORDER=1          LJ Verlet rows ordered by LDS bank class at build time (an experiment)                      off
   double nlMargin;            // COMD_NL_MARGIN=x (0 <= x < 1) the deferred test's margin as a fraction of skin/2 (tests: force the stop); < 0 = unset     4 / list life
   int    skChunks;            // COMD_SK_CHUNKS=n (> 0)        atom chunks of computeStructureFactor, clamped to the local cells (tests: the sum over chunks)  fills the device
};
static ComdTuning readTuning()
{
   auto env = getenv;
   auto num = [&](const char* name) { const char* e = env(name); return e ? atoi(e) : 0; };                  // 0 when unset
   auto is = [&](const char* name, const char* value) { const char* e = env(name); return e && !strcmp(e, value); };
   auto isZero = [&](const char* name) { const char* e = env(name); return e && atoi(e) == 0; };             // set, and to 0
   auto shape = [&](const char* name, int* by, int* bz) { const char* e = env(name); if (!(e && sscanf(e, "%d,%d", by, bz) == 2 && *by >= 1 && *bz >= 1 && *by * *bz <= 64)) *by = *bz = 0; };
   ComdTuning t;
   t.nlGlobal = env("COMD_NL_GLOBAL") != nullptr;
   t.eamNlLds = is("COMD_EAM_NL", "lds");
   t.ljWaves = num("COMD_LJ_WAVES") > 0 ? num("COMD_LJ_WAVES") : 0;
   t.ljPrune = !isZero("COMD_LJ_PRUNE");
   t.ljPrefetch = !isZero("COMD_LJ_PREFETCH");
   t.ljListCap = num("COMD_LJ_LIST_CAP") > 0 ? (num("COMD_LJ_LIST_CAP") + 7) & ~7 : 0;
   t.ljListBudgetMb = env("COMD_LJ_LIST_BUDGET_MB") ? atof(env("COMD_LJ_LIST_BUDGET_MB")) : INFINITY;
   t.ljCtaSlabs = num("COMD_LJ_CTA_SLABS") != 0;
   t.eamCtaCell = is("COMD_EAM_CTA", "cell");
   t.eamThreadAtomCell = is("COMD_EAM_THREAD_ATOM", "cell");
   t.eamGroups = !isZero("COMD_EAM_GROUPS");
   shape("COMD_EAM_BRICK", &t.eamBrickBy, &t.eamBrickBz);
   t.eamImage = num("COMD_EAM_IMAGE") >= 64 ? (num("COMD_EAM_IMAGE") + 7) / 8 * 8 : 0;
   t.eamAblate = num("COMD_EAM_ABLATE");
   t.eamClamp = num("COMD_EAM_CLAMP") != 0;
   t.eamAtomRows = num("COMD_EAM_ATOM_ROWS") >= 8 && num("COMD_EAM_ATOM_ROWS") <= 128 ? num("COMD_EAM_ATOM_ROWS") / 8 * 8 : 0;
   t.eamAtomHandover = !isZero("COMD_EAM_ATOM_HANDOVER");
   shape("COMD_EAM_ATOM_BRICK", &t.eamAtomBrickBy, &t.eamAtomBrickBz);
   t.eamAtomLdsPad = num("COMD_EAM_ATOM_LDS_PAD");
   t.eamCtaWaves = num("COMD_EAM_CTA_WAVES") >= 1 && num("COMD_EAM_CTA_WAVES") <= 8 ? num("COMD_EAM_CTA_WAVES") : 0;
   t.eamStencil = num("COMD_EAM_STENCIL") >= 64 ? (num("COMD_EAM_STENCIL") + 7) / 8 * 8 : 0;
   t.nlSync = num("COMD_NL_SYNC") != 0;
   t.eamListsEveryBuild = env("COMD_EAM_LISTS_EVERY_BUILD") != nullptr;
   t.nlBankOrder = num("COMD_NL_BANK_ORDER") != 0;
   t.nlMargin = env("COMD_NL_MARGIN") && atof(env("COMD_NL_MARGIN")) >= 0.0 && atof(env("COMD_NL_MARGIN")) < 1.0 ? atof(env("COMD_NL_MARGIN")) : -1.0;
   t.skChunks = num("COMD_SK_CHUNKS") > 0 ? num("COMD_SK_CHUNKS") : 0;
   return t;
}
// AllocateGpu fills SimGpu.tuning; a SimGpu that reaches a launch wrapper without it gets its record here
static const ComdTuning& tuningOf(SimGpu* sim) { if (!sim->tuning) sim->tuning = new ComdTuning(readTuning()); return *(const ComdTuning*)sim->tuning; }
// ---- what the last force launches ran (comdForceLegReport): written down by the launch wrappers, per simulation, SimGpu.legs ----
struct ForceLegs {
   int ljWaves, ljListCap, ljLists, ljCtaForm, ljPrefetch;
   int eamKernel, eamBy, eamBz, eamImage, eamBricks, eamPass1Grid, eamRows, eamPass3ReadsRows, eamCover, eamRunMax, eamTablesInLds, eamSpline, eamClampsKept, eamStencil;
};
static ForceLegs& legsOf(SimGpu* sim) { if (!sim->legs) sim->legs = new ForceLegs(); return *(ForceLegs*)sim->legs; }
// The density estimates behind the sizing of rows, lists and LDS images: the perfect FCC lattice, 4 atoms per lat^3 (GpuConfig.latticeConstant; 0: copper)
static double latticeConstantOf(const SimGpu* sim) { return sim->latticeConstant > 0.0 ? sim->latticeConstant : 3.615; }
static const double SPHERE_VOLUME = 4.18879020478639;      // of radius 1


// ---- force-kernel timing (bench.py roofline leg): per simulation, SimGpu.timing -----------------------------------
// Two classes of launches are timed apart: kind 0 the force kernels proper (the kernel the roofline object names), kind 1 what a force
// evaluation launches beside them (LJ thread_atom: LJ_PackPositions + LJ_WaveCandidates; the cell marks of a list launch).  A force
// EVALUATION costs the sum of the two.
struct ForceTiming {
   struct Ev { hipEvent_t a, b; int kind; };
   std::vector<Ev> pool;
   size_t used = 0;
   double ms[2] = { 0.0, 0.0 };
   int launches[2] = { 0, 0 };
   bool on = false;
};

static void timingFlush(ForceTiming* t)
{
   if (!t) return;
   for (size_t i = 0; i < t->used; ++i) {
      float ms = 0.f;
      HIP_CHECK(hipEventSynchronize(t->pool[i].b));
      HIP_CHECK(hipEventElapsedTime(&ms, t->pool[i].a, t->pool[i].b));
      t->ms[t->pool[i].kind] += ms;
      t->launches[t->pool[i].kind] += 1;
   }
   t->used = 0;
}

struct ForceTimer {
   ForceTiming* t; hipStream_t st; int idx;
   ForceTimer(SimGpu* sim, hipStream_t s, int kind = 0) : t((ForceTiming*)sim->timing), st(s), idx(-1)
   {
      if (!t || !t->on) return;
      if (t->used == t->pool.size()) {
         if (t->pool.size() >= 1024) timingFlush(t);
         else { hipEvent_t a, b; HIP_CHECK(hipEventCreate(&a)); HIP_CHECK(hipEventCreate(&b)); t->pool.push_back({a, b, 0}); }
      }
      idx = (int)t->used++;
      t->pool[idx].kind = kind;
      HIP_CHECK(hipEventRecord(t->pool[idx].a, st));
   }
   ~ForceTimer() { if (idx >= 0) HIP_CHECK(hipEventRecord(t->pool[idx].b, st)); }
};

extern "C" void comdForceTimingEnable(SimGpu* sim, int on)
{
   if (!sim->timing) { if (!on) return; sim->timing = new ForceTiming(); }
   ((ForceTiming*)sim->timing)->on = on != 0;
}
extern "C" void comdForceTimingReset(SimGpu* sim)
{
   ForceTiming* t = (ForceTiming*)sim->timing;
   if (!t) return;
   timingFlush(t); t->ms[0] = t->ms[1] = 0.0; t->launches[0] = t->launches[1] = 0;
}
extern "C" double comdForceTimingTotalMs(SimGpu* sim, int* nLaunches)
{
   ForceTiming* t = (ForceTiming*)sim->timing;
   if (!t) { if (nLaunches) *nLaunches = 0; return 0.0; }
   timingFlush(t);
   if (nLaunches) *nLaunches = t->launches[0];
   return t->ms[0];
}
extern "C" double comdForceTimingAuxMs(SimGpu* sim, int* nLaunches)
{
   ForceTiming* t = (ForceTiming*)sim->timing;
   if (!t) { if (nLaunches) *nLaunches = 0; return 0.0; }
   timingFlush(t);
   if (nLaunches) *nLaunches = t->launches[1];
   return t->ms[1];
}

extern "C" void comdDeviceMemInfo(long* freeBytes, long* totalBytes)
{
   size_t f = 0, tot = 0;
   HIP_CHECK(hipMemGetInfo(&f, &tot));
   if (freeBytes) *freeBytes = (long)f;
   if (totalBytes) *totalBytes = (long)tot;
}

extern "C" void* comdEventCreate(void) { hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); return (void*)e; }
extern "C" void comdEventRecord(void* ev, comdStream_t stream) { HIP_CHECK(hipEventRecord((hipEvent_t)ev, S(stream))); }
extern "C" float comdEventElapsedMs(void* start, void* stop)
{
   float ms = 0.f;
   HIP_CHECK(hipEventSynchronize((hipEvent_t)stop));
   HIP_CHECK(hipEventElapsedTime(&ms, (hipEvent_t)start, (hipEvent_t)stop));
   return ms;
}
extern "C" void comdEventDestroy(void* ev) { HIP_CHECK(hipEventDestroy((hipEvent_t)ev)); }
extern "C" void comdEventSynchronize(void* ev) { HIP_CHECK(hipEventSynchronize((hipEvent_t)ev)); }

// ---- device management ---------------------------------------------------------------------------------------
extern "C" int comdDeviceCount(void)
{
   int n = 0;
   if (hipGetDeviceCount(&n) != hipSuccess) return 0;
   return n;
}

extern "C" int SetupGpu(int deviceId, int rank, int verbose)
{
   g_rank = rank;
   HIP_CHECK(hipSetDevice(deviceId));
   hipDeviceProp_t props;
   HIP_CHECK(hipGetDeviceProperties(&props, deviceId));
   if (verbose)
      printf("Rank %d: device %d = %s (%s), %d CUs, %.1f GiB\n", rank, deviceId, props.name, props.gcnArchName,
             props.multiProcessorCount, props.totalGlobalMem / 1073741824.0);
   return props.multiProcessorCount;
}

extern "C" void comdDeviceSynchronize(void) { HIP_CHECK(hipDeviceSynchronize()); }
extern "C" void comdStreamSynchronize(comdStream_t stream) { HIP_CHECK(hipStreamSynchronize(S(stream))); }
extern "C" void* comdDeviceMalloc(long bytes) { void* p = nullptr; HIP_CHECK(hipMalloc(&p, (size_t)(bytes > 0 ? bytes : 8))); return p; }
extern "C" void comdDeviceFree(void* p) { if (p) HIP_CHECK(hipFree(p)); }
extern "C" void* comdHostMallocPinned(long bytes) { void* p = nullptr; HIP_CHECK(hipHostMalloc(&p, (size_t)(bytes > 0 ? bytes : 8), hipHostMallocDefault)); return p; }
extern "C" void comdHostFreePinned(void* p) { if (p) HIP_CHECK(hipHostFree(p)); }
extern "C" void comdMemcpyHtoD(void* dst, const void* src, long bytes) { HIP_CHECK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice)); }
extern "C" void comdMemcpyDtoH(void* dst, const void* src, long bytes) { HIP_CHECK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost)); }
extern "C" void comdMemcpyDtoDAsync(void* dst, const void* src, long bytes, comdStream_t stream)
{
   HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, S(stream)));
}

extern "C" void comdMemcpyAsync(void* dst, const void* src, long bytes, int kind, comdStream_t stream)
{
   if (bytes <= 0) return;
   const hipMemcpyKind k = kind == 1 ? hipMemcpyHostToDevice : kind == 2 ? hipMemcpyDeviceToHost : kind == 3 ? hipMemcpyDeviceToDevice : hipMemcpyHostToHost;
   HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)bytes, k, S(stream)));
}
// cudaMemset of the reference's host files (timestep.c:224): issued on the legacy default stream, which waits for and is waited for by the reference's
// streams (created with flags 0, gpu_utility.c:150-152).  The -a 1 streams here are non-blocking, so the same ordering is spelled out.
extern "C" void comdDeviceMemset(void* p, int value, long bytes)
{
   if (bytes <= 0) return;
   HIP_CHECK(hipDeviceSynchronize());
   HIP_CHECK(hipMemset(p, value, (size_t)bytes));
   HIP_CHECK(hipDeviceSynchronize());
}

template <typename T> static T* dalloc(size_t n, bool zero = true)
{
   T* p = nullptr;
   HIP_CHECK(hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)));
   if (zero) HIP_CHECK(hipMemset(p, 0, (n ? n : 1) * sizeof(T)));
   return p;
}

// tailPad: entries past the n + 3 of the table (the LJ table has one, see comdLjInterpolationTable)
static void uploadTable(InterpolationObjectGpu* t, int n, real_t x0, real_t invDx, const real_t* hostValues, int tailPad = 0)
{
   t->n = n; t->x0 = x0; t->invDx = invDx;
   t->xn = x0 + n / invDx;                     // gpu_utility.c:446, 460-461
   t->invDxHalf = invDx * 0.5;
   t->invDxXx0 = x0 * invDx;
   if (!t->values) t->values = dalloc<real_t>((size_t)n + 3 + tailPad, false);
   HIP_CHECK(hipMemcpy(t->values, hostValues, ((size_t)n + 3 + tailPad) * sizeof(real_t), hipMemcpyHostToDevice));
}

// The -I table (gpu_utility.c:349-372), restated with the reference's types and order of operations so that every sample is the reference's to the
// bit: the expressions with 1.0 are evaluated in double in the single-precision build as well, and nothing is contracted into an fma.
extern "C" int comdLjInterpolationTable(real_t sigma, real_t epsilon, real_t cutoff, real_t* x0, real_t* invDx, real_t* values)
{
#pragma clang fp contract(off)
   const int n = 1000;
   const real_t tx0 = 0.5 * sigma;
   const real_t tinv = n / (cutoff - tx0);
   if (x0) *x0 = tx0;
   if (invDx) *invDx = tinv;
   if (!values) return n;
   const real_t rCut2 = cutoff * cutoff;
   const real_t s6 = sigma * sigma * sigma * sigma * sigma * sigma;
   const real_t rCut6 = s6 / (rCut2 * rCut2 * rCut2);
   const real_t eShift = rCut6 * (rCut6 - 1.0);
   for (int i = 0; i < n + 3; ++i) {
      const real_t x = tx0 + (i - 1) / tinv;
      const real_t r2 = 1.0 / (x * x);
      const real_t r6 = s6 * r2 * r2 * r2;
      values[i] = 4 * epsilon * (r6 * (r6 - 1.0) - eShift);
   }
   values[n + 3] = values[n + 2];      // a pair at r == xn reads v[n + 3]: one past the reference's array
   return n;
}

extern "C" void initLJinterpolation(LjPotentialGpu* pot)
{
   real_t x0, invDx;
   const int n = comdLjInterpolationTable(pot->sigma, pot->epsilon, pot->cutoff, &x0, &invDx, nullptr);
   std::vector<real_t> v((size_t)n + 4);
   comdLjInterpolationTable(pot->sigma, pot->epsilon, pot->cutoff, &x0, &invDx, v.data());
   uploadTable(&pot->lj_interpolation, n, x0, invDx, v.data(), 1);
}

extern "C" void initLinkCellsGpu(LinkCellGpu* b, const GpuConfig* cfg)
{
   b->nLocalBoxes = cfg->nLocalBoxes; b->nTotalBoxes = cfg->nTotalBoxes;
   for (int a = 0; a < 3; ++a) {
      b->gridSize[a] = cfg->gridSize[a]; b->localMin[a] = cfg->localMin[a]; b->localMax[a] = cfg->localMax[a];
      b->invBoxSize[a] = 1.0 / cfg->boxSize[a];
   }
   b->nAtoms = dalloc<int>(cfg->nTotalBoxes);
   b->boxIDLookUp = b->boxIDLookUpReverse = nullptr;
   if (cfg->boxIDLookUp && cfg->boxIDLookUpReverse) {     // gpu_utility.c:594-595
      b->boxIDLookUp = dalloc<int>(cfg->nLocalBoxes, false);
      b->boxIDLookUpReverse = dalloc<int>(cfg->nLocalBoxes, false);
      HIP_CHECK(hipMemcpy(b->boxIDLookUp, cfg->boxIDLookUp, (size_t)cfg->nLocalBoxes * sizeof(int), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(b->boxIDLookUpReverse, cfg->boxIDLookUpReverse, (size_t)cfg->nLocalBoxes * sizeof(int), hipMemcpyHostToDevice));
   }
}

extern "C" void AllocateGpu(SimGpu* sim, const GpuConfig* cfg)
{
   memset(sim, 0, sizeof(*sim));
   HIP_CHECK(hipGetDevice(&sim->deviceId));
   sim->rank = cfg->rank; g_rank = cfg->rank;
   sim->maxAtoms = cfg->maxAtoms;
   sim->needEnergy = 1;
   sim->latticeConstant = cfg->latticeConstant;
   {  // (the expression the launch layer evaluated on LinkCellGpu.invBoxSize at every launch while the box could not change)
      const real_t i0 = 1.0 / cfg->boxSize[0], i1 = 1.0 / cfg->boxSize[1], i2 = 1.0 / cfg->boxSize[2];
      sim->cellVolume0 = 1.0 / (i0 * i1 * i2);
   }
   sim->do_eam = cfg->do_eam;
   sim->mass = cfg->mass;
   const ComdTuning& tune = tuningOf(sim);
   if (cfg->maxAtoms < 1 || cfg->maxAtoms > 1024) { fprintf(stderr, "AllocateGpu: maxAtoms %d outside [1,1024]\n", cfg->maxAtoms); exit(-1); }
   if (!cfg->do_eam && (cfg->maxAtoms % 64) != 0) { fprintf(stderr, "AllocateGpu: LJ needs maxAtoms %% 64 == 0 (got %d)\n", cfg->maxAtoms); exit(-1); }

   initLinkCellsGpu(&sim->boxes, cfg);
   const size_t slots = (size_t)cfg->nTotalBoxes * cfg->maxAtoms;      // 64-bit: 256^3 LJ needs 136 M slots
   AtomsGpu* at = &sim->atoms;
   at->r.x = dalloc<real_t>(slots); at->r.y = dalloc<real_t>(slots); at->r.z = dalloc<real_t>(slots);
   at->p.x = dalloc<real_t>(slots); at->p.y = dalloc<real_t>(slots); at->p.z = dalloc<real_t>(slots);
   at->f.x = dalloc<real_t>(slots); at->f.y = dalloc<real_t>(slots); at->f.z = dalloc<real_t>(slots);
   at->e = dalloc<real_t>(slots);
   at->iSpecies = dalloc<int>(slots); at->gid = dalloc<int>(slots);
   sim->neighbor_cells = dalloc<int>((size_t)cfg->nLocalBoxes * 27, false);
   HIP_CHECK(hipMemcpy(sim->neighbor_cells, cfg->neighborCells, (size_t)cfg->nLocalBoxes * 27 * sizeof(int), hipMemcpyHostToDevice));
   sim->species_mass = dalloc<real_t>(1, false);
   HIP_CHECK(hipMemcpy(sim->species_mass, &cfg->mass, sizeof(real_t), hipMemcpyHostToDevice));

   sim->lj_pot.cutoff = cfg->ljCutoff; sim->lj_pot.sigma = cfg->ljSigma; sim->lj_pot.epsilon = cfg->ljEpsilon;
   if (!cfg->do_eam && cfg->ljTableValues)        // -I (gpu_utility.c:509-510)
      uploadTable(&sim->lj_pot.lj_interpolation, cfg->ljTableN, cfg->ljTableX0, cfg->ljTableInvDx, cfg->ljTableValues, 1);
   if (cfg->do_eam) {
      sim->eam_pot.cutoff = cfg->eamCutoff;
      uploadTable(&sim->eam_pot.phi, cfg->nPhi, cfg->phiX0, cfg->phiInvDx, cfg->phiValues);
      uploadTable(&sim->eam_pot.rho, cfg->nRho, cfg->rhoX0, cfg->rhoInvDx, cfg->rhoValues);
      uploadTable(&sim->eam_pot.f,   cfg->nF,   cfg->fX0,   cfg->fInvDx,   cfg->fValues);
      if (cfg->phiSpline && cfg->rhoSpline) {             // gpu_utility.c:247-249, 478-500
         auto up = [](InterpolationSplineObjectGpu* t, int n, real_t x0, real_t invDx, const real_t* host) {
            t->n = n; t->x0 = (float)x0; t->xn = (float)(x0 + n / invDx); t->invDx = (float)invDx; t->invDxXx0 = (float)(invDx * x0);
            t->coefficients = dalloc<real_t>((size_t)4 * n, false);
            HIP_CHECK(hipMemcpy(t->coefficients, host, (size_t)4 * n * sizeof(real_t), hipMemcpyHostToDevice));
         };
         up(&sim->eam_pot.phiS, cfg->nPhi, cfg->phiX0, cfg->phiInvDx, cfg->phiSpline);
         up(&sim->eam_pot.rhoS, cfg->nRho, cfg->rhoX0, cfg->rhoInvDx, cfg->rhoSpline);
      }
      sim->eam_pot.rhobar = dalloc<real_t>(slots);
      sim->eam_pot.dfEmbed = dalloc<real_t>(slots);
   }
   if (cfg->skinDistance > 0.0) {               // gpu_neighborList.c:49-86 initNeighborListGpu
      NeighborListGpu* nl = &at->neighborList;
      const real_t cutoff = cfg->do_eam ? cfg->eamCutoff : cfg->ljCutoff;
      nl->skinDistance = cfg->skinDistance; nl->skinDistance2 = cfg->skinDistance * cfg->skinDistance;
      nl->skinDistanceHalf2 = 0.25 * nl->skinDistance2;
      nl->maxNeighbors = cfg->maxNeighbors;
      if (nl->maxNeighbors <= 0) {
         // atoms inside the list sphere at the perfect-lattice density (4 per lat^3), + 20 % and 24 for thermal crowding
         const double rl = cutoff + cfg->skinDistance, lat = latticeConstantOf(sim);
         const double expect = 4.0 / (lat * lat * lat) * SPHERE_VOLUME * rl * rl * rl;
         nl->maxNeighbors = ((int)(1.2 * expect) + 24 + 7) / 8 * 8;
      }
      if (nl->maxNeighbors > 27 * cfg->maxAtoms) nl->maxNeighbors = 27 * cfg->maxAtoms;
      const size_t localSlots = (size_t)cfg->nLocalBoxes * cfg->maxAtoms;
      nl->slabFormat = !cfg->usePairlist && !cfg->do_eam && cfg->maxAtoms % 64 == 0 && cfg->maxAtoms <= 512 && !tune.nlGlobal;
      if (cfg->usePairlist) {
         if (cfg->do_eam) { fprintf(stderr, "AllocateGpu: pairlists (-L) are an LJ cta_cell feature\n"); exit(-1); }
         nl->slabFormat = 3;
         const int threads = cfg->maxAtoms < 256 ? cfg->maxAtoms : 256;
         nl->pairlistWaves = (threads + 63) / 64;
         nl->pairlist = dalloc<unsigned>((size_t)cfg->nLocalBoxes * nl->pairlistWaves * LJ_CTA_SLABS * LJ_PL_WORDS);
         nl->pairlistBuildId = -1;
      } else if (cfg->do_eam && !tune.nlGlobal && !tune.eamNlLds
                 && (double)cfg->nTotalBoxes * cfg->maxAtoms * sizeof(real_t) < 4294967296.0) {
         // [round 4] EAM: rows of the brick kernel (eam_brick_kernels.h, LISTED): 16-bit record numbers in the LDS image of the atom's brick, kept from one
         // list build to the next.  Any table size (setfl tables and -P coefficients are read through L2), any cell capacity.
         nl->slabFormat = 4;
         nl->brickRowLen = (nl->maxNeighbors + 7) / 8 * 8;
         if (nl->brickRowLen > 2 * EAM_LIST_WORDS * 16) nl->brickRowLen = 2 * EAM_LIST_WORDS * 16;      // 16 lanes x 12 words x 2 numbers
         const int lanesMin = (nl->brickRowLen + 2 * EAM_LIST_WORDS - 1) / (2 * EAM_LIST_WORDS);          // as the kernel derives them from `rows`
         nl->brickRoundAtoms = 64 / lanesMin < 16 ? 64 / lanesMin : 16;
         nl->brickRounds = (cfg->maxAtoms + nl->brickRoundAtoms - 1) / nl->brickRoundAtoms;
         const int lanesPerAtom = 64 / nl->brickRoundAtoms;                                                // the fewest lanes an atom is ever dealt to
         int words = (nl->brickRowLen / 2 + lanesPerAtom - 1) / lanesPerAtom;
         if (words > EAM_LIST_WORDS) words = EAM_LIST_WORDS;
         nl->brickQuads = (words + 3) / 4;
         nl->brickRows = dalloc<unsigned>((size_t)cfg->nLocalBoxes * nl->brickRounds * nl->brickQuads * 64 * 4, false);
         nl->brickRowCount = dalloc<unsigned short>(localSlots);
      } else if (cfg->do_eam && cfg->maxAtoms <= 64 && eamCtaTableBytes(1, cfg->nRho, cfg->nPhi) <= 32 * 1024 && !tune.nlGlobal) {
         // EAM with LDS-sized tables: 16-bit entries into the wave's staging of the whole 27-cell stencil
         nl->slabFormat = 2;
         nl->slabRows = nl->maxNeighbors;
         nl->list16 = dalloc<unsigned short>(localSlots * nl->slabRows, false);
         nl->nNeighbors = dalloc<int>(localSlots);
         nl->stats = dalloc<int>(2);
      } else if (nl->slabFormat) {
         // share of the list sphere (radius R) one group can hold.  3 groups: the atom's own x-plane of cells, thickness wx, cuts at
         // most wx * pi R^2 out of 4/3 pi R^3 (78 % for cells of about R); 9 groups: its own z-column, wx * wy * 2R (51 %)
         const double R = cutoff + cfg->skinDistance;
         double share = NL_DIAGONAL ? 0.62                     // own cell + edge cells; measured 0.44-0.5 of the list for cells of about R
                      : NL_GROUPS == 3 ? 3.0 * cfg->boxSize[0] / (4.0 * R)
                                       : 3.0 * cfg->boxSize[0] * cfg->boxSize[1] / (2.0 * 3.14159265358979 * R * R);
         if (share > 1.0) share = 1.0;
         nl->slabRows = ((int)(share * nl->maxNeighbors) + 7) / 8 * 8;
         if (nl->slabRows > NL_GROUP_CELLS * cfg->maxAtoms) nl->slabRows = NL_GROUP_CELLS * cfg->maxAtoms;
         nl->list16 = dalloc<unsigned short>(localSlots * NL_GROUPS * nl->slabRows, false);
         nl->nNeighbors = dalloc<int>(localSlots * NL_GROUPS);
         nl->stats = dalloc<int>(2);
      } else {
         nl->list = dalloc<int>(localSlots * nl->maxNeighbors, false);
         nl->nNeighbors = dalloc<int>(localSlots);
      }
      nl->lastR.x = dalloc<real_t>(localSlots); nl->lastR.y = dalloc<real_t>(localSlots); nl->lastR.z = dalloc<real_t>(localSlots);
      HIP_CHECK(hipHostMalloc((void**)&nl->updateRequiredHost, 64, hipHostMallocDefault));      // pinned: written by kernels, read by the host
      memset(nl->updateRequiredHost, 0, 64);
      HIP_CHECK(hipHostGetDevicePointer((void**)&nl->updateRequired, nl->updateRequiredHost, 0));
      nl->forceRebuildFlag = 1; nl->nBuilds = 0;
   }
   sim->nAtomsPrev = dalloc<int>(cfg->nTotalBoxes);
   sim->cellDirty = dalloc<int>(cfg->nTotalBoxes);
   sim->cellArrivals = dalloc<int>((size_t)3 * cfg->nTotalBoxes);
   sim->d_updateLinkCellsRequired = dalloc<int>(1);
   sim->status = dalloc<int>(4);
   sim->reduceBlocks = 1024;
   sim->reduceBuf = dalloc<real_t>(2 * (size_t)sim->reduceBlocks + 2);
   HIP_CHECK(hipHostMalloc((void**)&sim->pinned, 64 * sizeof(real_t), hipHostMallocDefault));
   memset(sim->pinned, 0, 64 * sizeof(real_t));
   HIP_CHECK(hipHostGetDevicePointer((void**)&sim->statusMirrorDev, (int*)(sim->pinned + 32), 0));

   if (cfg->gpuAsync) {                         // gpu_utility.c:150-159
      hipStream_t bs, is;
      int lo = 0, hi = 0;
      HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
      HIP_CHECK(hipStreamCreateWithPriority(&bs, hipStreamNonBlocking, hi));
      HIP_CHECK(hipStreamCreateWithFlags(&is, hipStreamNonBlocking));
      sim->boundary_stream = (comdStream_t)bs; sim->interior_stream = (comdStream_t)is;
   } else {
      sim->boundary_stream = nullptr; sim->interior_stream = nullptr;
   }
   HIP_CHECK(hipDeviceSynchronize());            // the zeroing above is done before any non-blocking stream can touch these arrays
}

extern "C" void SetBoundaryCells(SimGpu* sim, int nBoundary, const int* boundary, int nInterior, const int* interior,
                                 int nBoundary1, const int* boundary1)
{
   sim->n_boundary_cells = nBoundary; sim->n_interior_cells = nInterior; sim->n_boundary1_cells = nBoundary1;
   sim->boundary_cells = dalloc<int>(nBoundary, false);
   sim->interior_cells = dalloc<int>(nInterior, false);
   sim->boundary1_cells = dalloc<int>(nBoundary1, false);
   if (nBoundary)  HIP_CHECK(hipMemcpy(sim->boundary_cells, boundary, (size_t)nBoundary * sizeof(int), hipMemcpyHostToDevice));
   if (nInterior)  HIP_CHECK(hipMemcpy(sim->interior_cells, interior, (size_t)nInterior * sizeof(int), hipMemcpyHostToDevice));
   if (nBoundary1) HIP_CHECK(hipMemcpy(sim->boundary1_cells, boundary1, (size_t)nBoundary1 * sizeof(int), hipMemcpyHostToDevice));
}

extern "C" void CopyDataToGpu(SimGpu* sim, const HostAtoms* h)
{
   const size_t slots = (size_t)sim->boxes.nTotalBoxes * sim->maxAtoms;
   sim->max_atoms_cell = 0;                       // unknown until the next updateNAtomsCpu: launch cap/64 waves per cell
   HIP_CHECK(hipMemcpy(sim->boxes.nAtoms, h->nAtoms, (size_t)sim->boxes.nTotalBoxes * sizeof(int), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(sim->atoms.gid, h->gid, slots * sizeof(int), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(sim->atoms.iSpecies, h->iSpecies, slots * sizeof(int), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(sim->atoms.r.x, h->rx, slots * sizeof(real_t), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(sim->atoms.r.y, h->ry, slots * sizeof(real_t), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(sim->atoms.r.z, h->rz, slots * sizeof(real_t), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(sim->atoms.p.x, h->px, slots * sizeof(real_t), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(sim->atoms.p.y, h->py, slots * sizeof(real_t), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(sim->atoms.p.z, h->pz, slots * sizeof(real_t), hipMemcpyHostToDevice));
}

extern "C" void GetDataFromGpu(SimGpu* sim, HostAtoms* h)
{
   HIP_CHECK(hipDeviceSynchronize());
   const size_t slots = (size_t)sim->boxes.nTotalBoxes * sim->maxAtoms;
   HIP_CHECK(hipMemcpy(h->nAtoms, sim->boxes.nAtoms, (size_t)sim->boxes.nTotalBoxes * sizeof(int), hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemcpy(h->gid, sim->atoms.gid, slots * sizeof(int), hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemcpy(h->iSpecies, sim->atoms.iSpecies, slots * sizeof(int), hipMemcpyDeviceToHost));
   real_t* dst[10] = { h->rx, h->ry, h->rz, h->px, h->py, h->pz, h->fx, h->fy, h->fz, h->e };
   real_t* src[10] = { sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z,
                       sim->atoms.f.x, sim->atoms.f.y, sim->atoms.f.z, sim->atoms.e };
   for (int i = 0; i < 10; ++i) if (dst[i]) HIP_CHECK(hipMemcpy(dst[i], src[i], slots * sizeof(real_t), hipMemcpyDeviceToHost));
}

extern "C" void updateNAtomsCpu(SimGpu* sim, int* nAtomsHost)
{
   HIP_CHECK(hipDeviceSynchronize());
   HIP_CHECK(hipMemcpy(nAtomsHost, sim->boxes.nAtoms, (size_t)sim->boxes.nTotalBoxes * sizeof(int), hipMemcpyDeviceToHost));
   int m = 0;
   for (int i = 0; i < sim->boxes.nTotalBoxes; ++i) if (nAtomsHost[i] > m) m = nAtomsHost[i];
   sim->max_atoms_cell = m;                       // gpu_types.h:160 max_atoms_cell: sizes the LJ thread_atom workgroups
}

// gpu_utility.h:60-69, the rest of the staging surface (the reference's cpu_nl path moves atoms between its host arrays and the device with these)
extern "C" void cudaCopyDtH(void* dst, const void* src, int size) { HIP_CHECK(hipMemcpy(dst, src, (size_t)size, hipMemcpyDeviceToHost)); }      // gpu_utility.c:46-49, same signature

extern "C" void GetLocalAtomsFromGpu(SimGpu* sim, HostAtoms* h)                     // gpu_utility.c:656-673: momenta, positions and gids of the LOCAL cells
{
   HIP_CHECK(hipDeviceSynchronize());
   const size_t slots = (size_t)sim->boxes.nLocalBoxes * sim->maxAtoms;
   real_t* dst[6] = { h->px, h->py, h->pz, h->rx, h->ry, h->rz };
   real_t* src[6] = { sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z, sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z };
   for (int i = 0; i < 6; ++i) if (dst[i]) HIP_CHECK(hipMemcpy(dst[i], src[i], slots * sizeof(real_t), hipMemcpyDeviceToHost));
   if (h->gid) HIP_CHECK(hipMemcpy(h->gid, sim->atoms.gid, slots * sizeof(int), hipMemcpyDeviceToHost));
}

extern "C" void updateGpuHalo(SimGpu* sim, const HostAtoms* h)                       // gpu_utility.c:714-757: the HALO cells' slots, host -> device
{
   const size_t first = (size_t)sim->boxes.nLocalBoxes * sim->maxAtoms, slots = (size_t)(sim->boxes.nTotalBoxes - sim->boxes.nLocalBoxes) * sim->maxAtoms;
   const real_t* src[6] = { h->px, h->py, h->pz, h->rx, h->ry, h->rz };
   real_t* dst[6] = { sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z, sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z };
   for (int i = 0; i < 6; ++i) HIP_CHECK(hipMemcpy(dst[i] + first, src[i] + first, slots * sizeof(real_t), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(sim->atoms.gid + first, h->gid + first, slots * sizeof(int), hipMemcpyHostToDevice));
   HIP_CHECK(hipMemcpy(sim->atoms.iSpecies + first, h->iSpecies + first, slots * sizeof(int), hipMemcpyHostToDevice));
}

extern "C" void updateNAtomsGpu(SimGpu* sim, const int* nAtomsHost)                  // gpu_utility.c:602-605
{
   HIP_CHECK(hipMemcpy(sim->boxes.nAtoms, nAtomsHost, (size_t)sim->boxes.nTotalBoxes * sizeof(int), hipMemcpyHostToDevice));
}

// gpu_utility.c:678-712, a host loop there as here: the atoms of the halo cells, cell by cell, as one SoA message in h_compactAtoms (no header);
// h_cellOffset[i] = atoms in the halo cells before the i-th, nHalo + 1 entries.  (The reference zeroes h_cellOffset[nLocalBoxes] instead of [0] and
// relies on the caller's calloc; entry 0 is written here.)
extern "C" int compactHaloCells(const HostAtoms* h, int nLocalBoxes, int nTotalBoxes, int maxAtoms, char* h_compactAtoms, int* h_cellOffset)
{
   const int nHalo = nTotalBoxes - nLocalBoxes;
   h_cellOffset[0] = 0;
   for (int i = 0; i < nHalo; ++i) h_cellOffset[i + 1] = h_cellOffset[i] + h->nAtoms[nLocalBoxes + i];
   const int n = h_cellOffset[nHalo];
   int* gid = (int*)h_compactAtoms; int* type = gid + n;
   real_t* m = (real_t*)(type + n);
   for (int i = 0; i < nHalo; ++i) {
      size_t o = (size_t)(nLocalBoxes + i) * maxAtoms;
      for (int k = h_cellOffset[i]; k < h_cellOffset[i + 1]; ++k, ++o) {
         gid[k] = h->gid[o]; type[k] = h->iSpecies[o];
         m[k] = h->rx[o]; m[(size_t)n + k] = h->ry[o]; m[2 * (size_t)n + k] = h->rz[o];
         m[3 * (size_t)n + k] = h->px[o]; m[4 * (size_t)n + k] = h->py[o]; m[5 * (size_t)n + k] = h->pz[o];
      }
   }
   return n;
}

extern "C" void DestroyGpu(SimGpu* sim)
{
   HIP_CHECK(hipDeviceSynchronize());
   if (sim->timing) {
      ForceTiming* t = (ForceTiming*)sim->timing;
      timingFlush(t);
      for (auto& ev : t->pool) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
      delete t;
   }
   delete (ComdTuning*)sim->tuning;
   delete (ForceLegs*)sim->legs;
   void* ptrs[] = { sim->boxes.nAtoms, sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z,
                    sim->atoms.f.x, sim->atoms.f.y, sim->atoms.f.z, sim->atoms.e, sim->atoms.iSpecies, sim->atoms.gid,
                    sim->neighbor_cells, sim->species_mass, sim->eam_pot.phi.values, sim->eam_pot.rho.values, sim->eam_pot.f.values,
                    sim->eam_pot.rhobar, sim->eam_pot.dfEmbed, sim->nAtomsPrev, sim->cellDirty, sim->cellArrivals, sim->d_updateLinkCellsRequired, sim->status, sim->reduceBuf,
                    sim->boundary_cells, sim->interior_cells, sim->boundary1_cells,
                    sim->atoms.neighborList.list, sim->atoms.neighborList.nNeighbors, sim->atoms.neighborList.lastR.x,
                    sim->atoms.neighborList.lastR.y, sim->atoms.neighborList.lastR.z,
                    sim->atoms.neighborList.list16, sim->atoms.neighborList.stats, sim->atoms.neighborList.pairlist,
                    sim->boxes.boxIDLookUp, sim->boxes.boxIDLookUpReverse, sim->eam_pot.phiS.coefficients, sim->eam_pot.rhoS.coefficients,
                    sim->eam_pot.pairRows, sim->eam_pot.pairRowCount, sim->eam_pot.cellSel, sim->eam_pot.brickGroup, sim->eam_pot.brickList, sim->eam_pot.brickSel, sim->eam_pot.brickStats, sim->eam_pot.atomRows, sim->eam_pot.atomRowCount, sim->eam_pot.atomBrickSel,
                    sim->atoms.neighborList.brickRows, sim->atoms.neighborList.brickRowCount, sim->adapterScan, sim->lj_pot.waveCand, sim->lj_pot.waveCandCount, sim->lj_pot.packedR[0], sim->lj_pot.packedR[1], sim->lj_pot.packedF[0], sim->lj_pot.packedF[1],
                    sim->lj_pot.lj_interpolation.values, sim->virialBuf, sim->pairHistBuf, sim->dispBuf, sim->dispSumBuf, sim->cspBuf, sim->cspCoordBuf, sim->cnaBuf, sim->stressBuf, sim->stressSumBuf,
                    sim->strainRefBuf, sim->strainBuf, sim->strainCountBuf, sim->strainSumBuf, sim->heatFluxBuf, sim->heatFluxSumBuf, sim->fdotrBuf, sim->fdotrRows, sim->profileBuf, sim->mpBuf, sim->mpRows, sim->skBuf, sim->steinhardtBuf, sim->steinhardtSumBuf, sim->bornBuf };
   for (void* p : ptrs) if (p) HIP_CHECK(hipFree(p));
   if (sim->statusEvent) (void)hipEventDestroy((hipEvent_t)sim->statusEvent);
   if (sim->pinned) HIP_CHECK(hipHostFree(sim->pinned));
   if (sim->atoms.neighborList.updateRequiredHost) HIP_CHECK(hipHostFree(sim->atoms.neighborList.updateRequiredHost));
   if (sim->atoms.neighborList.brickStatsMirror) HIP_CHECK(hipHostFree(sim->atoms.neighborList.brickStatsMirror));
   if (sim->atoms.neighborList.brickStatsEvent) (void)hipEventDestroy((hipEvent_t)sim->atoms.neighborList.brickStatsEvent);
   if (sim->boundary_stream) HIP_CHECK(hipStreamDestroy(S(sim->boundary_stream)));
   if (sim->interior_stream) HIP_CHECK(hipStreamDestroy(S(sim->interior_stream)));
   memset(sim, 0, sizeof(*sim));
}

extern "C" void emptyHaloCellsGpu(SimGpu* sim, comdStream_t stream)
{
   const int nHalo = sim->boxes.nTotalBoxes - sim->boxes.nLocalBoxes;
   HIP_CHECK(hipMemsetAsync(sim->boxes.nAtoms + sim->boxes.nLocalBoxes, 0, (size_t)nHalo * sizeof(int), S(stream)));
}

extern "C" void comdCheckStatus(SimGpu* sim, const char* where)
{
   int st[4];
   HIP_CHECK(hipDeviceSynchronize());
   HIP_CHECK(hipMemcpy(st, sim->status, sizeof st, hipMemcpyDeviceToHost));
   if (st[0] | st[1] | st[2] | st[3]) {
      fprintf(stderr, "Rank %d, GPU: %d, %s: ", g_rank, sim->deviceId, where);
      if (st[0] & 1) fprintf(stderr, "a link cell overflowed its %d slots (raise --maxAtoms); ", sim->maxAtoms);
      if (st[0] & 2) fprintf(stderr, "a cell stencil holds more atoms than the cta_cell kernel can stage; ");
      if (st[1])     fprintf(stderr, "an atom moved beyond the halo region and was lost; ");
      if (st[2])     fprintf(stderr, "a halo message overflowed its buffer, or grew by more than 12.5 %% + 64 atoms in one step (COMD_HALO_HANDSHAKE=1 exchanges exact sizes); ");
      if (st[3] & 1) fprintf(stderr, "an atom has more neighbours inside the cutoff than a row of the EAM cta_cell kernel holds (1.5 x the FCC count; use -m thread_atom); ");
      if (st[3] & 2) fprintf(stderr, "an atom has more than %d neighbours inside cutoff + skin (raise --maxNeighbors); ", sim->atoms.neighborList.maxNeighbors);
      if (st[3] & 4) fprintf(stderr, "eamForce3Gpu[Async] covered the cells with another partition than eamForce1Gpu[Async] (include/comd_hip.h: same lists in both passes); ");
      fprintf(stderr, "\n");
      exit(-1);
   }
}

extern "C" void comdPollStatus(SimGpu* sim, comdStream_t stream, const char* where)
{
   int* mirror = (int*)(sim->pinned + 32);               // four ints of the 64-real_t pinned block, away from the energy words
   // [round 4] The fused drift kernels copy the status words into the mirror as they start (step_kernels.h skinProgress): nothing to enqueue here -- the separate
   // 16-byte copy per step was a blit kernel with a launch gap on either side, 10 us of every step.  Without such a kernel since the last poll: the copy, as before.
   if (sim->statusMirrored) {
      sim->statusMirrored = 0;
      if (mirror[0] | mirror[1] | mirror[2] | mirror[3]) comdCheckStatus(sim, where);
      return;
   }
   if (sim->statusEvent) {
      if (hipEventQuery((hipEvent_t)sim->statusEvent) != hipSuccess) return;       // the previous mirror has not landed yet: look again next step
      if (mirror[0] | mirror[1] | mirror[2] | mirror[3]) comdCheckStatus(sim, where);
   } else {
      hipEvent_t e; HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); sim->statusEvent = (void*)e;
   }
   HIP_CHECK(hipMemcpyAsync(mirror, sim->status, 4 * sizeof(int), hipMemcpyDeviceToHost, S(stream)));
   HIP_CHECK(hipEventRecord((hipEvent_t)sim->statusEvent, S(stream)));
}

extern "C" int comdReadDeviceInt(const int* d_ptr, comdStream_t stream)
{
   int v = 0;
   HIP_CHECK(hipMemcpyAsync(&v, d_ptr, sizeof(int), hipMemcpyDeviceToHost, S(stream)));
   HIP_CHECK(hipStreamSynchronize(S(stream)));
   return v;
}

// ---- force -------------------------------------------------------------------------------------------------------
// Per-atom energies are consumed only by computeEnergy.  The host announces with comdSetEnergyNeeded(0) that the coming
// force evaluations feed no energy read (all but the last step of a timestep() call); the default is 1 (always compute).
extern "C" void comdSetEnergyNeeded(SimGpu* sim, int on) { sim->needEnergy = on; }

#include "lj_launch.h"       // the LJ launch layer: nlView, makeLjArgs ... ljForceGpu
#include "eam_launch.h"      // the EAM launch layer: makeEamArgs ... eamForce3Gpu

// what the force wrappers decided for this simulation (bench.py records it beside the numbers): {LJ thread_atom candidate lists in use (0: the 27-cell walk),
// records of the EAM brick image, Verlet-list format (comd_hip.h slabFormat), cells per EAM brick}
extern "C" void comdForcePathInfo(SimGpu* sim, int out[4])
{
   out[0] = sim->lj_pot.packedCap > 0 ? 1 : 0;
   out[1] = sim->eam_pot.brickImageCap ? sim->eam_pot.brickImageCap : sim->eam_pot.atomBrickImageCap;
   out[2] = sim->atoms.neighborList.slabFormat;
   out[3] = (sim->eam_pot.brickBy ? sim->eam_pot.brickBy * sim->eam_pot.brickBz : sim->eam_pot.atomBrickBy * sim->eam_pot.atomBrickBz) + 256 * sim->eam_pot.brickListMakes;      // (cells per brick in the low byte, times the brick lists were made above)
}

extern "C" void comdOverlapCellCounts(SimGpu* sim, int out[3])
{
   out[0] = sim->n_boundary_cells; out[1] = sim->n_interior_cells; out[2] = sim->n_boundary1_cells;
}

// what the last force evaluation ran (comd_hip.h has the entries): host records of the launch wrappers, and counts taken from waveCandCount / brickStats as they stand
extern "C" void comdForceLegReport(SimGpu* sim, int out[COMD_LEG_REPORT_N])
{
   for (int k = 0; k < COMD_LEG_REPORT_N; ++k) out[k] = 0;
   HIP_CHECK(hipDeviceSynchronize());
   const ForceLegs& g = legsOf(sim);
   const LjPotentialGpu* lj = &sim->lj_pot;
   out[0] = g.ljWaves; out[1] = g.ljListCap; out[2] = g.ljLists; out[7] = g.ljCtaForm;
   if (g.ljWaves > 0) {
      // a wave per 64-atom chunk of a local cell; LJ_WaveCandidates leaves {own-cell, all} candidates (all == -1: walk) for chunk < min(waves per cell, waveCandWaves)
      const int nCells = sim->boxes.nLocalBoxes, wavesMax = lj->waveCandWaves;
      std::vector<int> counts((size_t)nCells), cand;
      HIP_CHECK(hipMemcpy(counts.data(), sim->boxes.nAtoms, counts.size() * sizeof(int), hipMemcpyDeviceToHost));
      if (g.ljLists && lj->waveCandCount) {
         cand.resize((size_t)nCells * wavesMax * 2);
         HIP_CHECK(hipMemcpy(cand.data(), lj->waveCandCount, cand.size() * sizeof(int), hipMemcpyDeviceToHost));
      }
      int listed = 0, walked = 0, lo = 0, hi = 0;
      int full = 0, fullOdd = 0, fullOddSelf = 0, fullLo = 0;       // the listed waves of more than 32 atoms: the ones that run ljListLoop
      for (int c = 0; c < nCells; ++c) {
         const int chunks = (counts[c] + 63) / 64;
         for (int k = 0; k < chunks; ++k) {
            const int n = (!cand.empty() && k < g.ljWaves && k < wavesMax) ? cand[((size_t)c * wavesMax + k) * 2 + 1] : -1;
            if (n < 0) { ++walked; continue; }
            if (!listed || n < lo) lo = n;
            if (!listed || n > hi) hi = n;
            ++listed;
            if (counts[c] - 64 * k > 32) {
               if (!full || n < fullLo) fullLo = n;
               ++full;
               if (n % 64) ++fullOdd;
               if (cand[((size_t)c * wavesMax + k) * 2] % 8) ++fullOddSelf;
            }
         }
      }
      out[3] = listed; out[4] = walked; out[5] = lo; out[6] = hi;
      out[25] = full; out[26] = fullOdd; out[27] = fullOddSelf; out[28] = fullLo; out[29] = LJ_PREFETCH_D;
   }
   out[8] = g.eamKernel; out[9] = g.eamBy; out[10] = g.eamBz; out[11] = g.eamImage; out[12] = g.eamBricks; out[13] = g.eamPass1Grid;
   if (sim->eam_pot.brickStats) HIP_CHECK(hipMemcpy(&out[14], sim->eam_pot.brickStats + 2, sizeof(int), hipMemcpyDeviceToHost));
   out[15] = g.eamRows; out[16] = g.eamPass3ReadsRows; out[17] = g.eamCover; out[18] = g.eamRunMax; out[19] = g.eamTablesInLds; out[20] = g.eamSpline;
   out[21] = g.eamClampsKept; out[22] = g.eamStencil; out[23] = sim->atoms.neighborList.slabFormat; out[24] = g.ljPrefetch;
   // Verlet rows: the entries a row holds in this format, and the longest row the last build left (the counts the force kernels read: clamped to the capacity)
   const NeighborListGpu* n = &sim->atoms.neighborList;
   const int fmt = n->slabFormat, nCells = sim->boxes.nLocalBoxes, cap = sim->maxAtoms;
   const int groups = fmt == 1 ? NL_GROUPS : 1;
   out[30] = fmt == 4 ? n->brickRowLen : (fmt == 1 || fmt == 2) ? n->slabRows : (fmt == 0 && n->list) ? n->maxNeighbors : 0;
   if (n->nBuilds > 0 && (fmt == 4 ? n->brickRowCount != nullptr : fmt != 3 && n->nNeighbors != nullptr)) {
      const size_t slots = (size_t)nCells * groups * cap;
      std::vector<int> counts((size_t)nCells), len(slots);
      HIP_CHECK(hipMemcpy(counts.data(), sim->boxes.nAtoms, counts.size() * sizeof(int), hipMemcpyDeviceToHost));
      if (fmt == 4) {
         std::vector<unsigned short> len16(slots);
         HIP_CHECK(hipMemcpy(len16.data(), n->brickRowCount, slots * sizeof(unsigned short), hipMemcpyDeviceToHost));
         for (size_t s = 0; s < slots; ++s) len[s] = len16[s];
      } else HIP_CHECK(hipMemcpy(len.data(), n->nNeighbors, slots * sizeof(int), hipMemcpyDeviceToHost));
      int longest = 0;
      for (int c = 0; c < nCells; ++c)
         for (int g2 = 0; g2 < groups; ++g2)
            for (int i = 0; i < counts[c] && i < cap; ++i) { const int v = len[((size_t)c * groups + g2) * cap + i]; if (v > longest) longest = v; }
      out[31] = longest;
   }
}

extern "C" void updateNeighborsGpu(SimGpu*, int*) {}
extern "C" void updateNeighborsGpuAsync(SimGpu*, int*, int, int*, comdStream_t) {}

// ---- integrator + energy -----------------------------------------------------------------------------------------
// lanes of a 256-thread workgroup that serve one cell in the integrator kernels (step_kernels.h COMD_CELL_SLOTS): the power of two that covers the usual occupancy of a
// cell of this capacity -- capacities are the lattice maximum + 10 % + 8, and cells hold about a third of that (EAM) or 60 % (LJ, multiples of 64)
static int integratorLaneBits(const SimGpu* sim)
{
   const int cap = sim->maxAtoms;
   return cap <= 48 ? 4 : cap <= 96 ? 5 : cap <= 192 ? 6 : 8;
}
static dim3 integratorGrid(const SimGpu* sim) { return dim3((unsigned)ceilDiv(sim->boxes.nLocalBoxes, 256 >> integratorLaneBits(sim))); }

extern "C" void advanceVelocityGpu(SimGpu* sim, real_t dt)
{
   const long slots = (long)sim->boxes.nLocalBoxes * sim->maxAtoms;
   hipLaunchKernelGGL(AdvanceVelocity, integratorGrid(sim), dim3(256), 0, S(sim->boundary_stream),
                      sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z, sim->atoms.f.x, sim->atoms.f.y, sim->atoms.f.z,
                      sim->boxes.nAtoms, sim->boxes.nLocalBoxes, sim->maxAtoms, dt, integratorLaneBits(sim));
   LAUNCH_CHECK();
}

// displacement tracking (msd_kernels.h): what the drift kernels add into; d == NULL while comdTrackDisplacementGpu has not switched it on
static DispTrack dispTrackOf(const SimGpu* sim) { DispTrack t = { (long long*)sim->dispBuf, sim->dispN }; return t; }

extern "C" void advancePositionGpu(SimGpu* sim, real_t dt)
{
   const long slots = (long)sim->boxes.nLocalBoxes * sim->maxAtoms;
   hipLaunchKernelGGL(AdvancePosition, integratorGrid(sim), dim3(256), 0, S(sim->boundary_stream),
                      sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z,
                      sim->atoms.iSpecies, sim->species_mass, sim->boxes.nAtoms, sim->boxes.nLocalBoxes, sim->maxAtoms, dt, sim->atoms.gid, dispTrackOf(sim),
                      integratorLaneBits(sim));
   LAUNCH_CHECK();
}

// Verlet lists: the fused drift kernels test the displacement since the list build as they write the new positions (step_kernels.h SkinCheck);
// neighborListUpdateRequiredGpu then only reads the flag.  No lists, or none built yet: nothing to check.
static SkinCheck skinCheckOf(SimGpu* sim)
{
   NeighborListGpu* n = &sim->atoms.neighborList;
   SkinCheck sk = { nullptr, nullptr, nullptr, R(0.0), R(0.0), nullptr, nullptr, nullptr, 0, sim->status, sim->statusMirrorDev };
   sim->statusMirrored = 1;
   if (!n->lastR.x || n->nBuilds == 0 || n->forceRebuildFlag) return sk;
   sk.lastX = n->lastR.x; sk.lastY = n->lastR.y; sk.lastZ = n->lastR.z; sk.skinHalf2 = n->skinDistanceHalf2;
   sk.softHalf2 = n->softHalf2 > R(0.0) ? n->softHalf2 : n->skinDistanceHalf2;
   if (n->affineBudget > R(0.0) && n->affineBudget < R(1.0)) {      // a box compressed since the build has eaten into the skin (comdSetListBudgetGpu)
      const real_t b2 = n->affineBudget * n->affineBudget;
      sk.skinHalf2 *= b2; sk.softHalf2 *= b2;
   }
   sk.hard = n->updateRequired + 1; sk.soft = n->updateRequired + 2; sk.progress = n->updateRequired + 3; sk.stamp = ++n->driftCount;
   n->checkFused = 1;
   return sk;
}
extern "C" void advanceVelocityPositionGpu(SimGpu* sim, real_t dtKick, real_t dtDrift)
{
   const long slots = (long)sim->boxes.nLocalBoxes * sim->maxAtoms;
   const SkinCheck sk = skinCheckOf(sim);
   hipLaunchKernelGGL(AdvanceVelocityPosition, integratorGrid(sim), dim3(256), 0, S(sim->boundary_stream),
                      sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z,
                      sim->atoms.f.x, sim->atoms.f.y, sim->atoms.f.z, sim->atoms.iSpecies, sim->species_mass,
                      sim->boxes.nAtoms, sim->boxes.nLocalBoxes, sim->maxAtoms, dtKick, dtDrift, sk, sim->atoms.gid, dispTrackOf(sim),
                      integratorLaneBits(sim));
   LAUNCH_CHECK();
}

extern "C" void advanceVelocityVelocityPositionGpu(SimGpu* sim, real_t dtKick1, real_t dtKick2, real_t dtDrift)
{
   const long slots = (long)sim->boxes.nLocalBoxes * sim->maxAtoms;
   const SkinCheck sk = skinCheckOf(sim);
   hipLaunchKernelGGL(AdvanceVelocityVelocityPosition, integratorGrid(sim), dim3(256), 0, S(sim->boundary_stream),
                      sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z,
                      sim->atoms.f.x, sim->atoms.f.y, sim->atoms.f.z, sim->atoms.iSpecies, sim->species_mass,
                      sim->boxes.nAtoms, sim->boxes.nLocalBoxes, sim->maxAtoms, dtKick1, dtKick2, dtDrift, sk, sim->atoms.gid,
                      dispTrackOf(sim), integratorLaneBits(sim));
   LAUNCH_CHECK();
}

// BAOAB Langevin forms of the two launches above (langevin_kernels.h; no counterpart in the reference): same grid, stream and skin check
static LangevinO langevinOf(real_t c1, real_t c2, real_t kT, uint64_t seed, uint64_t step)
{
   LangevinO o = { c1, c2, kT, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(step >> 32) };
   return o;
}

extern "C" void advanceVelocityPositionLangevinGpu(SimGpu* sim, real_t dtKick, real_t dtHalfDrift, real_t c1, real_t c2, real_t kT,
                                                   uint64_t seed, uint64_t step)
{
   const SkinCheck sk = skinCheckOf(sim);
   hipLaunchKernelGGL(AdvanceVelocityPositionLangevin, integratorGrid(sim), dim3(256), 0, S(sim->boundary_stream),
                      sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z,
                      sim->atoms.f.x, sim->atoms.f.y, sim->atoms.f.z, sim->atoms.iSpecies, sim->atoms.gid, sim->species_mass,
                      sim->boxes.nAtoms, sim->boxes.nLocalBoxes, sim->maxAtoms, dtKick, dtHalfDrift, langevinOf(c1, c2, kT, seed, step), sk,
                      dispTrackOf(sim), integratorLaneBits(sim));
   LAUNCH_CHECK();
}

extern "C" void advanceVelocityVelocityPositionLangevinGpu(SimGpu* sim, real_t dtKick1, real_t dtKick2, real_t dtHalfDrift, real_t c1, real_t c2,
                                                           real_t kT, uint64_t seed, uint64_t step)
{
   const SkinCheck sk = skinCheckOf(sim);
   hipLaunchKernelGGL(AdvanceVelocityVelocityPositionLangevin, integratorGrid(sim), dim3(256), 0, S(sim->boundary_stream),
                      sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z,
                      sim->atoms.f.x, sim->atoms.f.y, sim->atoms.f.z, sim->atoms.iSpecies, sim->atoms.gid, sim->species_mass,
                      sim->boxes.nAtoms, sim->boxes.nLocalBoxes, sim->maxAtoms, dtKick1, dtKick2, dtHalfDrift, langevinOf(c1, c2, kT, seed, step),
                      sk, dispTrackOf(sim), integratorLaneBits(sim));
   LAUNCH_CHECK();
}

// Not in the reference: the affine remap of the positions to a new box (deform_kernels.h) and the device copy of the geometry that goes with it.  Lists built:
// their snapshot lastR is scaled in the same pass.  Grid sizes, capacities and cell lists do not change; whatever the kernels derive from the geometry
// (ljBoxMargins, the geometry of the EAM bricks, the packed positions of LJ thread_atom) is derived from sim->boxes at every launch.
extern "C" void comdRemapBoxGpu(SimGpu* sim, const double scale[3], const real_t localMin[3], const real_t localMax[3], const real_t boxSize[3], comdStream_t stream)
{
   NeighborListGpu* n = &sim->atoms.neighborList;
   RemapSnapshot last = { nullptr, nullptr, nullptr };
   if (n->lastR.x && n->nBuilds > 0) { last.x = n->lastR.x; last.y = n->lastR.y; last.z = n->lastR.z; }
   hipLaunchKernelGGL(RemapBox, integratorGrid(sim), dim3(256), 0, S(stream), sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, last,
                      sim->boxes.nAtoms, sim->boxes.nLocalBoxes, sim->maxAtoms, (real_t)scale[0], (real_t)scale[1], (real_t)scale[2], integratorLaneBits(sim));
   LAUNCH_CHECK();
   for (int a = 0; a < 3; ++a) {
      sim->boxes.localMin[a] = localMin[a]; sim->boxes.localMax[a] = localMax[a];
      sim->boxes.invBoxSize[a] = 1.0 / boxSize[a];
   }
}

// Verlet lists under a changing box: `budget` in (0, 1] is the share of skin/2 that is left for the non-affine motion of an atom once the compression of the box
// since the build has been paid for, (skin - e_c (rc + skin)) / skin; the hard and the soft threshold of the skin test are scaled by it.
// 1 (and the value after every build): the reference's rule, bit for bit.
extern "C" void comdSetListBudgetGpu(SimGpu* sim, double budget)
{
   sim->atoms.neighborList.affineBudget = budget >= 1.0 ? R(1.0) : (real_t)budget;
}

extern "C" void computeEnergy(SimGpu* sim, real_t* eLocal)
{
   hipStream_t st = S(sim->boundary_stream);
   const long slots = (long)sim->boxes.nLocalBoxes * sim->maxAtoms;
   int blocks = ceilDiv(slots, 256);
   if (blocks > sim->reduceBlocks) blocks = sim->reduceBlocks;
   real_t* out = sim->reduceBuf + 2 * (size_t)sim->reduceBlocks;
   hipLaunchKernelGGL(ReduceEnergyPartial, dim3(blocks), dim3(256), 0, st, sim->atoms.e, sim->atoms.p.x, sim->atoms.p.y, sim->atoms.p.z,
                      sim->atoms.iSpecies, sim->species_mass, sim->boxes.nAtoms, sim->boxes.nLocalBoxes, sim->maxAtoms, sim->reduceBuf);
   hipLaunchKernelGGL(ReduceEnergyFinal, dim3(1), dim3(256), 0, st, sim->reduceBuf, blocks, out);
   LAUNCH_CHECK();
   HIP_CHECK(hipMemcpyAsync(sim->pinned, out, 2 * sizeof(real_t), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
   eLocal[0] = sim->pinned[0]; eLocal[1] = sim->pinned[1];
}

#include "analysis_launch.h"      // the launch layer of the analyses: computeVirial ... comdMullerPlatheApplyGpu

// ---- redistribute ---------------------------------------------------------------------------------------------------
static AtomArrays atomArrays(SimGpu* sim)
{
   AtomArrays at;
   at.rx = sim->atoms.r.x; at.ry = sim->atoms.r.y; at.rz = sim->atoms.r.z;
   at.px = sim->atoms.p.x; at.py = sim->atoms.p.y; at.pz = sim->atoms.p.z;
   at.gid = sim->atoms.gid; at.spec = sim->atoms.iSpecies;
   return at;
}

static int sortBlock(int cap) { return ((cap + 63) / 64) * 64; }

static void launchCompactSort(SimGpu* sim, int first, int nCells, hipStream_t st, bool shortRuns = false)
{
   if (nCells <= 0) return;
   // cells per wave / workgroup: the local cells are nearly all clean (one flag each), the halo cells were all just refilled
   const bool halo = shortRuns || first >= sim->boxes.nLocalBoxes;
   if (sim->maxAtoms <= 64) {
      const int run = halo ? 2 : COMPACT_RUN_WAVE;
      hipLaunchKernelGGL(CompactSortCellsWave, dim3(ceilDiv(nCells, 4 * run)), dim3(256), 0, st,
                         atomArrays(sim), sim->boxes.nAtoms, sim->cellDirty, first, nCells, sim->maxAtoms, run, sim->cellArrivals, sim->boxes.nTotalBoxes);
      LAUNCH_CHECK();
      return;
   }
   const int run = halo ? 1 : COMPACT_RUN;
   hipLaunchKernelGGL(CompactSortCells, dim3(ceilDiv(nCells, run)), dim3(sortBlock(sim->maxAtoms)), (size_t)sortBlock(sim->maxAtoms) * sizeof(int), st,
                      atomArrays(sim), sim->boxes.nAtoms, sim->cellDirty, sim->status, first, nCells, sim->maxAtoms, run, sim->cellArrivals, sim->boxes.nTotalBoxes);
   LAUNCH_CHECK();
}

extern "C" void updateLinkCellsGpu(SimGpu* sim, comdStream_t stream)
{
   hipStream_t st = S(stream);
   const int nLocal = sim->boxes.nLocalBoxes, nTotal = sim->boxes.nTotalBoxes;
   hipLaunchKernelGGL(SnapshotCells, dim3(ceilDiv(nTotal, 256)), dim3(256), 0, st, sim->boxes.nAtoms, sim->nAtomsPrev, sim->cellDirty, sim->cellArrivals, nLocal, nTotal);
   hipLaunchKernelGGL(UpdateLinkCells, dim3(ceilDiv((long)nLocal * sim->maxAtoms, 256)), dim3(256), 0, st,
                      atomArrays(sim), sim->boxes.nAtoms, sim->nAtomsPrev, sim->cellDirty, sim->status, sim->boxes, sim->maxAtoms);
   LAUNCH_CHECK();
   // local cells that lost/gained atoms and halo cells that caught migrants -- unless the host says nothing needs them compact before sortAtomsGpu (every axis of the atom
   // exchange mirrored, which skips holes, and no interior force launch in between: SimGpu.skipSortAfterUpdate)
   if (!sim->skipSortAfterUpdate) launchCompactSort(sim, 0, nTotal, st);
}

extern "C" void buildAtomListGpu(SimGpu*, comdStream_t) {}

extern "C" void sortAtomsGpu(SimGpu* sim, comdStream_t stream)
{
   // after the atom exchange: local cells that received atoms (few) and the halo cells (all of them), one launch over all cells with the short runs of the halo
   // cells (round 3: two launches; a clean local cell costs its wave one flag read)
   launchCompactSort(sim, 0, sim->boxes.nTotalBoxes, S(stream), true);
}

// ---- halo pack / unpack ------------------------------------------------------------------------------------------------
#include "halo_launch.h"     // the halo launch layer: compactCellsGpu2 ... mirrorSlotCellsGpu

// ---- Verlet neighbour lists ------------------------------------------------------------------------------------------------
extern "C" void emptyNeighborListGpu(SimGpu* sim, int)
{
   NeighborListGpu* n = &sim->atoms.neighborList;
   if (n->nNeighbors) HIP_CHECK(hipMemsetAsync(n->nNeighbors, 0, (size_t)sim->boxes.nLocalBoxes * sim->maxAtoms * (n->slabFormat == 1 ? NL_GROUPS : 1) * sizeof(int), S(sim->boundary_stream)));
}

extern "C" void neighborListForceRebuildGpu(NeighborListGpu* nl) { nl->forceRebuildFlag = 1; }      // gpu_neighborList.c:88-93, same signature

extern "C" int neighborListUpdateRequiredGpu(SimGpu* sim)
{
   NeighborListGpu* n = &sim->atoms.neighborList;
   if ((!n->list && !n->list16 && !n->pairlist && !n->brickRows) || n->forceRebuildFlag) return 1;
   hipStream_t st = S(sim->boundary_stream);
   // The flags live in pinned host memory (the kernels write them there): a stream synchronisation and a host read, no copy.
   if (n->checkFused) {                                      // the drift kernel of the step checked the positions it wrote (step_kernels.h SkinCheck)
      n->checkFused = 0;
      HIP_CHECK(hipStreamSynchronize(st));
      return ((volatile int*)n->updateRequiredHost)[1] > n->buildDrift ? 1 : 0;
   }
   HIP_CHECK(hipStreamSynchronize(st));
   *n->updateRequiredHost = 0;                               // (raised only; cleared here, when nothing that writes it is in flight)
   hipLaunchKernelGGL(NeighborListUpdateRequired, dim3(ceilDiv((long)sim->boxes.nLocalBoxes * sim->maxAtoms, 256)), dim3(256), 0, st,
                      sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, n->lastR.x, n->lastR.y, n->lastR.z,
                      sim->boxes.nAtoms, sim->boxes.nLocalBoxes, sim->maxAtoms,
                      n->affineBudget > R(0.0) && n->affineBudget < R(1.0) ? n->skinDistanceHalf2 * n->affineBudget * n->affineBudget : n->skinDistanceHalf2, n->updateRequired);
   LAUNCH_CHECK();
   HIP_CHECK(hipStreamSynchronize(st));
   const int v = *(volatile int*)n->updateRequiredHost;
   *n->updateRequiredHost = 0;
   return v;
}

extern "C" int comdNeighborListUpdateDeferredGpu(SimGpu* sim)
{
   NeighborListGpu* n = &sim->atoms.neighborList;
   const bool forceSync = tuningOf(sim).nlSync;
   if (forceSync || !n->checkFused || n->forceRebuildFlag || n->lastInterval <= 0 || n->softHalf2 <= R(0.0)) return neighborListUpdateRequiredGpu(sim);
   n->checkFused = 0;
   const int G = n->driftCount, k = G - n->buildDrift;       // drift kernels so far, since the build
   const volatile int* f = (volatile int*)n->updateRequiredHost;
   // what drifts up to G - 2 found must be known: drift kernel G - 1 says so as it starts (f[3] = G - 2).  It has started long ago unless the host ran ahead of the
   // device by more than a step; then wait -- on the pinned word, not on the stream
   if (k >= 3) {
      long spins = 0;
      while (f[3] < G - 2) { __builtin_ia32_pause(); if (++spins > 200000000L) { HIP_CHECK(hipStreamSynchronize(S(sim->boundary_stream))); break; } }
   }
   const int hard = f[1], soft = f[2];
   if (hard > n->buildDrift && hard < G) {                   // the force evaluation behind drift `hard` used these lists beyond skin/2
      fprintf(stderr, "Rank %d: an atom moved more than skin/2 between two displacement tests of the deferred list check (margin %.1f %% of skin/2 after lists that lasted %d steps): "
                      "the neighbour lists were used beyond their validity.  COMD_NL_SYNC=1 tests every step before the force (blocking).\n",
              g_rank, 100.0 * (1.0 - sqrt((double)n->softHalf2 / (double)n->skinDistanceHalf2)), n->lastInterval);
      exit(-1);
   }
   return soft > n->buildDrift ? 1 : 0;
}

static void buildNeighborListImpl(SimGpu* sim, int method, int boundaryFlag)
{
   (void)method; (void)boundaryFlag;
   NeighborListGpu* n = &sim->atoms.neighborList;
   if (n->slabFormat == 3) {                   // pairlists: remember where the atoms are; the next force call generates the bits
      const size_t bytes = (size_t)sim->boxes.nLocalBoxes * sim->maxAtoms * sizeof(real_t);
      hipStream_t st = S(sim->boundary_stream);
      HIP_CHECK(hipMemcpyAsync(n->lastR.x, sim->atoms.r.x, bytes, hipMemcpyDeviceToDevice, st));
      HIP_CHECK(hipMemcpyAsync(n->lastR.y, sim->atoms.r.y, bytes, hipMemcpyDeviceToDevice, st));
      HIP_CHECK(hipMemcpyAsync(n->lastR.z, sim->atoms.r.z, bytes, hipMemcpyDeviceToDevice, st));
      n->forceRebuildFlag = 0;
      n->nBuilds++;
      return;
   }
   if (!n->list && !n->list16 && !n->brickRows) { fprintf(stderr, "buildNeighborListGpu: no lists allocated (GpuConfig.skinDistance == 0)\n"); exit(-1); }
   const real_t cutoff = sim->do_eam ? sim->eam_pot.cutoff : sim->lj_pot.cutoff;
   const real_t rBuild = cutoff + n->skinDistance;
   if (n->slabFormat == 4) {
      // rows of the brick kernel: the cells were just re-binned, so the image is sized again for the fullest block; STEP 0 sweeps every brick once
      hipStream_t st = S(sim->boundary_stream);
      // The brick lists (and the image size they were made for) are kept from build to build: making them costs the host a read-back of the occupancies and 1 ms in
      // which the device idles.  What tells when they are stale is the build kernel itself -- it counts the bricks whose block no longer fits the image (they take the
      // thread-per-atom form, correct and slow) -- read back asynchronously and looked at by the NEXT build, which then makes the lists again.
      if (!n->brickStatsMirror) { HIP_CHECK(hipHostMalloc((void**)&n->brickStatsMirror, 64, hipHostMallocDefault)); memset(n->brickStatsMirror, 0, 64); }
      if (n->brickStatsEvent) {
         HIP_CHECK(hipEventSynchronize((hipEvent_t)n->brickStatsEvent));      // recorded a whole list life ago
         if (n->brickStatsMirror[1] > 0) sim->eam_pot.brickListsValid = 0;
      }
      if (tuningOf(sim).eamListsEveryBuild) sim->eam_pot.brickListsValid = 0;      // (A/B runs, tests)
      if (!sim->eam_pot.brickListsValid) {
         eamBrickBuildLists(sim, st, sim->eam_pot.phiS.coefficients != nullptr);      // (sizes the image as well)
         sim->eam_pot.brickListsValid = 1;
      }
      EamArgs a = makeEamArgs(sim, sim->boxes.nLocalBoxes, nullptr);
      if (!sim->eam_pot.brickStats) sim->eam_pot.brickStats = dalloc<int>(3);
      HIP_CHECK(hipMemsetAsync(sim->eam_pot.brickStats, 0, 2 * sizeof(int), st));
      launchEamBrick<0>(sim, a, sim->boxes.nLocalBoxes, nullptr, st, EamTablePlan(a.phi, a.rho, 0), true, THREAD_ATOM_NL);
      LAUNCH_CHECK();
      HIP_CHECK(hipMemcpyAsync(n->brickStatsMirror, sim->eam_pot.brickStats, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
      if (!n->brickStatsEvent) { hipEvent_t e; HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); n->brickStatsEvent = (void*)e; }
      HIP_CHECK(hipEventRecord((hipEvent_t)n->brickStatsEvent, st));
      const size_t bytes = (size_t)sim->boxes.nLocalBoxes * sim->maxAtoms * sizeof(real_t);
      HIP_CHECK(hipMemcpyAsync(n->lastR.x, sim->atoms.r.x, bytes, hipMemcpyDeviceToDevice, st));
      HIP_CHECK(hipMemcpyAsync(n->lastR.y, sim->atoms.r.y, bytes, hipMemcpyDeviceToDevice, st));
      HIP_CHECK(hipMemcpyAsync(n->lastR.z, sim->atoms.r.z, bytes, hipMemcpyDeviceToDevice, st));
      n->forceRebuildFlag = 0;
      n->nBuilds++;
      return;
   }
   if (n->slabFormat) {
      hipStream_t st = S(sim->boundary_stream);
      NlSlabView sv; sv.list = n->list16; sv.count = n->nNeighbors; sv.rows = n->slabRows;
      HIP_CHECK(hipMemsetAsync(n->stats, 0, 2 * sizeof(int), st));
      if (n->slabFormat == 2) {
         // A wave stages a whole 27-cell stencil; the LDS it needs decides how many waves share a CU.  Worst case is 27 full cells
         // (1188 atoms at 44 slots: one workgroup per CU); what the last build saw (+25 %) is usually 2-3x less.  If a stencil does not
         // fit, the kernel says so through stats[0] and the build is repeated with the worst-case size.
         const int worst = 27 * sim->maxAtoms < 1536 ? 27 * sim->maxAtoms : 1536;
         int stencilCap = n->nBuilds > 0 && n->maxSlabAtoms > 0 ? n->maxSlabAtoms + n->maxSlabAtoms / 4 + 16 : worst;
         if (stencilCap > worst) stencilCap = worst;
         for (;;) {
            const size_t lds = (size_t)EAM_NL_WAVES * eamBuildWaveBytes(stencilCap, n->slabRows);
            allowDynamicLds((const void*)BuildNeighborListCell16, lds);
            HIP_CHECK(hipMemsetAsync(n->stats, 0, 2 * sizeof(int), st));
            hipLaunchKernelGGL(BuildNeighborListCell16, dim3(ceilDiv(sim->boxes.nLocalBoxes, EAM_NL_WAVES * 8)), dim3(64 * EAM_NL_WAVES), lds, st,
                               sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->boxes.nAtoms, sim->neighbor_cells,
                               sim->boxes.nLocalBoxes, sim->maxAtoms, sv, rBuild * rBuild, n->lastR.x, n->lastR.y, n->lastR.z, n->stats, sim->status, stencilCap);
            LAUNCH_CHECK();
            int h[2];
            HIP_CHECK(hipMemcpyAsync(h, n->stats, sizeof h, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            n->maxSlabAtoms = h[0]; n->maxCellAtoms = h[1] > 0 ? h[1] : 1;
            if (h[0] <= stencilCap || stencilCap == worst) break;
            stencilCap = worst;
         }
         n->forceRebuildFlag = 0;
         n->nBuilds++;
         return;
      } else
      {
         // one workgroup per cell, a thread per slot; the LDS holds a whole group of full cells (<= 9 * 512 atoms = 108 KB)
         // COMD_NL_BANK_ORDER=1: rows ordered by LDS bank class (nl_kernels.h): 2 x 16 counters of 16 bits per thread behind the records.  An experiment that settled a
         // question (profiles/r04_experiments/README.md): it takes 45 % of the bank-conflict cycles out of LJ_Force_nl_slabs and 1.3 % of its time -- the kernel is bound by
         // VALU issue, not by the LDS -- while the build goes from 11 to 79 ms.  Off by default.
         const int bankOrder = tuningOf(sim).nlBankOrder;
         const int groupCap = NL_GROUP_CELLS * sim->maxAtoms;
         const size_t lds = (size_t)3 * groupCap * sizeof(real_t) + (bankOrder ? (size_t)2 * 16 * sim->maxAtoms * sizeof(unsigned short) : 0);
         allowDynamicLds((const void*)BuildNeighborListSlabs, lds);
         hipLaunchKernelGGL(BuildNeighborListSlabs, dim3(sim->boxes.nLocalBoxes), dim3(sim->maxAtoms), lds, st,
                            sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->boxes.nAtoms, sim->neighbor_cells,
                            sim->boxes.nLocalBoxes, sim->maxAtoms, sv, rBuild * rBuild, n->lastR.x, n->lastR.y, n->lastR.z, n->stats, sim->status, bankOrder, groupCap);
      }
      LAUNCH_CHECK();
      int h[2];
      HIP_CHECK(hipMemcpyAsync(h, n->stats, sizeof h, hipMemcpyDeviceToHost, st));      // builds are rare: one blocking read each
      HIP_CHECK(hipStreamSynchronize(st));
      n->maxSlabAtoms = h[0]; n->maxCellAtoms = h[1] > 0 ? h[1] : 1;
      if (n->slabFormat == 1 && n->maxCellAtoms > 512) { fprintf(stderr, "buildNeighborListGpu: %d atoms in a cell, the slab kernel takes 512\n", n->maxCellAtoms); exit(-1); }
      n->forceRebuildFlag = 0;
      n->nBuilds++;
      return;
   }
   NlView v; v.list = n->list; v.count = n->nNeighbors; v.maxNbr = n->maxNeighbors;
   hipLaunchKernelGGL(BuildNeighborList, dim3(ceilDiv((long)sim->boxes.nLocalBoxes * sim->maxAtoms, 256)), dim3(256), 0, S(sim->boundary_stream),
                      sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->boxes.nAtoms, sim->neighbor_cells, (const int*)nullptr,
                      sim->boxes.nLocalBoxes, sim->maxAtoms, v, rBuild * rBuild, n->lastR.x, n->lastR.y, n->lastR.z, sim->status);
   LAUNCH_CHECK();
   n->forceRebuildFlag = 0;
   n->nBuilds++;
}

extern "C" void buildNeighborListGpu(SimGpu* sim, int method, int boundaryFlag)
{
   NeighborListGpu* n = &sim->atoms.neighborList;
   const int had = n->nBuilds;
   buildNeighborListImpl(sim, method, boundaryFlag);
   // bookkeeping of the deferred displacement test (comdNeighborListUpdateDeferredGpu): how long the previous lists lasted sizes the margin of these
   n->lastInterval = had > 0 ? n->driftCount - n->buildDrift : 0;
   n->buildDrift = n->driftCount;
   double frac = n->lastInterval > 0 ? 4.0 / n->lastInterval : 0.0;      // two steps' worth of twice the average growth per step
   if (frac < 0.1) frac = 0.1;
   if (frac > 0.6) frac = 0.6;
   if (tuningOf(sim).nlMargin >= 0.0) frac = tuningOf(sim).nlMargin;      // tests: force the stop
   n->softHalf2 = n->lastInterval > 0 ? (real_t)((1.0 - frac) * (1.0 - frac)) * n->skinDistanceHalf2 : R(0.0);
}

extern "C" int pairlistUpdateRequiredGpu(SimGpu* sim) { return neighborListUpdateRequiredGpu(sim); }
extern "C" void comdPairlistGenerated(SimGpu* sim) { sim->atoms.neighborList.pairlistBuildId = sim->atoms.neighborList.nBuilds; }

// the reference keeps a gid -> slot hash table for its list mode (hashTable.c); here atoms keep their slots between builds
extern "C" void initHashTableGpu(HashTableGpu* hashTable, int nMaxEntries) { if (hashTable) { hashTable->nMaxEntries = nMaxEntries; hashTable->nEntriesPut = hashTable->nEntriesGet = 0; } }
extern "C" void emptyHashTableGpu(HashTableGpu* hashTable) { if (hashTable) hashTable->nEntriesPut = hashTable->nEntriesGet = 0; }

// comm.h:40-74 (libmp / GPUDirect-Async): not part of this library -- "not in use" answers so that the reference's host objects take
// their plain send/receive path (haloExchange.c:726-730), which include/comd_hip.h serves through CommTransport
extern "C" int  comm_use_comm(void) { return 0; }
extern "C" int  comm_use_gdrdma(void) { return 0; }
extern "C" int  comm_use_async(void) { return 0; }
extern "C" int  comm_use_gpu_comm(void) { return 0; }
extern "C" int  comm_select_device(int mpiRank) { (void)mpiRank; return 0; }
extern "C" int  comm_init(...) { return 0; }
extern "C" void comm_finalize(void) {}

// The comm-layer-only part of the reference's link surface: defined so that its host objects link, never reachable while
// comm_use_comm() / comm_use_async() answer 0.  A call is a bug in the caller: say which symbol and stop.
#define COMD_ABSENT(name) extern "C" int name(...) { fprintf(stderr, "%s: the libmp / GPUDirect-Async layer is not part of this build (comm_use_comm() is 0)\n", #name); exit(-1); }
COMD_ABSENT(comm_irecv) COMD_ABSENT(comm_isend) COMD_ABSENT(comm_isend_on_stream) COMD_ABSENT(comm_send_ready) COMD_ABSENT(comm_send_ready_on_stream)
COMD_ABSENT(comm_wait_ready_on_stream) COMD_ABSENT(comm_wait_all) COMD_ABSENT(comm_wait_all_on_stream) COMD_ABSENT(comm_flush) COMD_ABSENT(comm_progress)
COMD_ABSENT(loadAtomsBufferFromGpu_Async) COMD_ABSENT(loadAtomsBufferFromGpu_Comm) COMD_ABSENT(unloadAtomsBufferToGpu_Async) COMD_ABSENT(unloadAtomsBufferToGpu_Comm)
COMD_ABSENT(loadForceBufferFromGpu_Async) COMD_ABSENT(loadForceBufferFromGpu_Comm) COMD_ABSENT(unloadForceBufferToGpu_Async) COMD_ABSENT(unloadForceBufferToGpu_Comm)
COMD_ABSENT(unloadForceScanCells) COMD_ABSENT(exchangeDataForceGpu_KI) COMD_ABSENT(neighborListUpdateRequiredGpu_Async)
#undef COMD_ABSENT
