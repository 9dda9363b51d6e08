/* cli.c -- the CoMD command line (mycommand.c:180-320 + cmdLineParser.c): same long names, same single-letter
 * flags, same defaults, same "Command Line Parameters" YAML block.  Table-driven over getopt_long.
 * Extensions (long options only): --maxAtoms N (link-cell slot capacity; the reference fixes it at
 * compile time with -DMAXATOMS), --maxNeighbors N (Verlet-list rows per atom for the *_nl methods; the reference's
 * MAXNEIGHBORLISTSIZE), --quiet, --ljCutoffSigmas F (the reference hard-wires 5; 2.5 meets its documented LJ cohesive energy),
 * --deviceTimers (also COMD_DEVICE_TIMERS=1: HIP-event timing of the phases in the reference's timer table),
 * --pressure (a Pressure(GPa) column in the report: pair virial + kinetic tensor, which the reference does not compute),
 * --langevin, --langevinTemp K, --langevinDamp FS, --seed N (BAOAB Langevin thermostat; the reference integrates NVE only),
 * --rdf N, --rdfMax R, --rdfFile PATH (radial distribution function g(r) from a pair histogram of N bins up to R Angstroms, sampled at every
 * printed step and written to PATH; the reference has no structural analysis),
 * --msd, --msdStart S, --msdFile PATH (mean-squared displacement of the unwrapped trajectories from global step S on, accumulated in the drift
 * kernels, sampled at every printed step and written to PATH with a diffusion coefficient; the reference has no dynamical analysis),
 * --csp, --cspThreshold X, --cspCoord R, --cspFile PATH, --cspDump PATH (per-atom defect analysis: the centro-symmetry parameter of every atom's 12
 * nearest neighbours and its coordination number within R Angstroms, sampled at every printed step; a Defects column counts the atoms above X
 * Angstroms^2, PATH gets a line per sample and the dump the defect atoms of the last step as extended XYZ),
 * --cna, --cnaFile PATH, --cnaDump PATH (adaptive common neighbour analysis: every atom is FCC, HCP, ICO or other, sampled at every printed step; a
 * NonFCC column, PATH gets the four counts per sample and the dump the non-FCC atoms of the last step as extended XYZ),
 * --erateX R, --erateY R, --erateZ R, --deformStart S, --deformFile PATH (box deformation: engineering strain rates in 1/ps applied from global step S on, the
 * positions remapped affinely at the top of every step; V/V0 and Sxx(GPa) columns, PATH gets strain, box and stress tensor per sample; the reference's box is fixed),
 * --baro, --baroP GPA, --baroTau FS, --baroModulus GPA, --baroEvery N, --baroAxes xyz, --baroIso, --baroStart S, --baroFile PATH (Berendsen barostat: every N steps the
 *   pressure from the forces of the step scales the chosen axes towards the target),
 * --profile, --profAxis x|y|z, --profBins N, --profStart S, --profFile PATH (slab profiles along one axis: count, temperature, kinetic and per-atom energy and mean
 *   velocity per slab, summed on the device in integers at every printed step from global step S on; PATH gets the time average),
 * --mp, --mpEvery N, --mpSwaps K, --mpStart S, --mpFile PATH (Mueller-Plathe reverse non-equilibrium exchange: every N steps the K hottest atoms of slab 0 and the K
 *   coldest of the middle slab swap momenta; turns --profile on, whose gradient gives the thermal conductivity; a dE(eV) column, PATH gets a row per exchange),
 * --stress, --stressFile PATH, --stressDump PATH, --stressDumpMin X (per-atom virial stress: hydrostatic pressure and von Mises stress of every atom with the
 * uniform atomic volume V/N, reduced on the device at every printed step; a MaxVM(GPa) column, PATH gets a line per sample and the dump the tensors of the atoms
 * of the last step whose von Mises stress is at least X GPa as extended XYZ; the reference has no stress output),
 * --strain, --strainRef S, --strainCutoff R, --strainThreshold X, --strainFile PATH, --strainDump PATH, --strainDumpMin X (per-atom strain against the state at
 * the end of global step S: the Green-Lagrange tensor of the best affine map of every atom's neighbourhood within R, its shear invariant and the non-affine
 * residue D^2min, reduced on the device at every printed step; a MaxShear column, PATH gets a line per sample and the dump the tensors of the atoms of the last
 * step whose shear strain is at least X as extended XYZ),
 * --heatflux, --hfStart S, --hfWindow M, --hfFile PATH, --hfAcfFile PATH (heat flux J V = sum_i (e_kin,i + e_i) v_i + 1/2 sum_i sum_j r_ij (f_ij . v_i), reduced on the
 * device at every printed step from global step S on; a Jx(eV/A^2/fs) column, PATH gets the samples, the ACF file the autocorrelation over M lags and the running
 * Green-Kubo thermal conductivity in W/(m K); the reference has no transport output),
 * --sk M, --skStride s|sx,sy,sz, --skBins N, --skStart S, --skFile PATH (static structure factor S(k) = |sum_j exp(-i k . r_j)|^2 / N on the half grid of wave vectors
 *   2 pi (sx h / Lx, sy k / Ly, sz l / Lz), h in [0, M], k, l in [-M, M], and the Bragg order S(111) / N of the conventional cell, summed on the device at every
 *   printed step from global step S on; an S111/N column, PATH gets the powder average over N |k| bins; the reference has no reciprocal-space analysis),
 * --steinhardt, --stSolid X, --stFile PATH, --stDump PATH, --stDumpMax X (Steinhardt's bond-orientational order q4, q6, w4, w6 of every atom on its 12 nearest
 *   neighbours, reduced on the device at every printed step; a MeanQ6 column, atoms with q6 >= X count as solid-like, PATH gets a line per sample and the dump the
 *   values of the atoms of the last step whose q6 is at most --stDumpMax, the invalid ones always, as extended XYZ),
 * --elastic, --elStart S, --elFile PATH (the Born matrix d^2 U / d eta d eta, summed on the device at every printed step from global step S on, and the
 *   stress-fluctuation elastic constants C = <B>/V - V/(kB T) cov(sigma) + N kB T/V kappa of the samples at the end of the run; a C11B(GPa) column, PATH gets a
 *   line per sample and the 6 x 6 C; a fixed box only: refused beside --erateX/Y/Z and --baro). */
#include "comd_host.h"
#include <getopt.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

typedef struct { const char* longName; char shortName; int hasArg; char type; void* ptr; int size; const char* help; } ArgDef;

static void printArgs(const ArgDef* defs, int n)
{
   fprintf(screenOut, "\n  Arguments are: \n");
   for (int i = 0; i < n; ++i) {
      char shortBuf[8] = "  ";
      if (defs[i].shortName > 0) snprintf(shortBuf, sizeof shortBuf, "-%c", defs[i].shortName);
      fprintf(screenOut, "   --%-20s %s  arg=%1d type=%c  %s\n", defs[i].longName, shortBuf, defs[i].hasArg, defs[i].type, defs[i].help);
   }
   fprintf(screenOut, "\n\n");
}

Command parseCommandLine(int argc, char** argv)
{
   Command cmd;
   memset(&cmd, 0, sizeof cmd);
   strcpy(cmd.potDir, "pots");
   strcpy(cmd.potType, "funcfl");
   strcpy(cmd.method, "thread_atom");
   cmd.nx = cmd.ny = cmd.nz = 20;
   cmd.xproc = cmd.yproc = cmd.zproc = 1;
   cmd.nSteps = 100; cmd.printRate = 10;
   cmd.ljCutoffSigmas = 5.0;
   cmd.dt = 1.0; cmd.lat = -1.0; cmd.temperature = 600.0; cmd.initialDelta = 0.0; cmd.relativeSkinDistance = 0.1;
   cmd.langevinTemp = NAN; cmd.langevinDamp = COMD_LANGEVIN_DAMP; cmd.seed = COMD_LANGEVIN_SEED;
   strcpy(cmd.rdfFile, "rdf.dat");
   strcpy(cmd.msdFile, "msd.dat");
   strcpy(cmd.cspFile, "csp.dat");
   strcpy(cmd.cnaFile, "cna.dat");
   strcpy(cmd.deformFile, "deform.dat");
   strcpy(cmd.stressFile, "stress.dat");
   strcpy(cmd.strainFile, "strain.dat");
   cmd.strainThreshold = 0.1;
   strcpy(cmd.hfFile, "heatflux.dat");
   strcpy(cmd.hfAcfFile, "hfacf.dat");
   cmd.baroTau = 1000.0; cmd.baroModulus = 140.0; cmd.baroEvery = 10;
   strcpy(cmd.baroAxes, "xyz");
   strcpy(cmd.baroFile, "baro.dat");
   strcpy(cmd.profAxis, "x"); cmd.profBins = 20;
   strcpy(cmd.profFile, "profile.dat");
   cmd.mpEvery = 100; cmd.mpSwaps = 1;
   strcpy(cmd.mpFile, "mp.dat");
   strcpy(cmd.skStride, "1"); cmd.skBins = 50;
   strcpy(cmd.skFile, "sk.dat");
   strcpy(cmd.stFile, "steinhardt.dat");
   cmd.stSolid = 0.45; cmd.stDumpMax = INFINITY;
   strcpy(cmd.elFile, "elastic.dat");
   int help = 0;

   const ArgDef defs[] = {
      { "help",         'h', 0, 'i', &help,               0, "print this message" },
      { "potDir",       'd', 1, 's', cmd.potDir,  sizeof cmd.potDir,  "potential directory" },
      { "potName",      'p', 1, 's', cmd.potName, sizeof cmd.potName, "potential name" },
      { "potType",      't', 1, 's', cmd.potType, sizeof cmd.potType, "potential type (funcfl or setfl)" },
      { "doeam",        'e', 0, 'i', &cmd.doeam,          0, "compute eam potentials" },
      { "nx",           'x', 1, 'i', &cmd.nx,             0, "number of unit cells in x" },
      { "ny",           'y', 1, 'i', &cmd.ny,             0, "number of unit cells in y" },
      { "nz",           'z', 1, 'i', &cmd.nz,             0, "number of unit cells in z" },
      { "xproc",        'i', 1, 'i', &cmd.xproc,          0, "processors in x direction" },
      { "yproc",        'j', 1, 'i', &cmd.yproc,          0, "processors in y direction" },
      { "zproc",        'k', 1, 'i', &cmd.zproc,          0, "processors in z direction" },
      { "nSteps",       'N', 1, 'i', &cmd.nSteps,         0, "number of time steps" },
      { "printRate",    'n', 1, 'i', &cmd.printRate,      0, "number of steps between output" },
      { "dt",           'D', 1, 'd', &cmd.dt,             0, "time step (in fs)" },
      { "lat",          'l', 1, 'd', &cmd.lat,            0, "lattice parameter (Angstroms)" },
      { "temp",         'T', 1, 'd', &cmd.temperature,    0, "initial temperature (K)" },
      { "delta",        'r', 1, 'd', &cmd.initialDelta,   0, "initial delta (Angstroms)" },
      { "hilbert",      'H', 0, 'i', &cmd.doHilbert,      0, "space-filling (Hilbert) curve for the numbering of the link cells" },
      { "skinDistance", 'S', 1, 'd', &cmd.relativeSkinDistance, 0, "skinDistance (relative to cutoff (default: 0.1))" },
      { "method",       'm', 1, 's', cmd.method,  sizeof cmd.method,  "thread_atom,thread_atom_nl,cta_cell (warp_atom[_nl] run as thread_atom[_nl])" },
      { "gpuAsync",     'a', 1, 'i', &cmd.gpuAsync,       0, "communicaton hiding optimization using streams" },
      { "gpuProfile",   's', 0, 'i', &cmd.gpuProfile,     0, "profiling mode: reboxing disabled, single kernel run" },
      { "ljInterpolation", 'I', 0, 'i', &cmd.ljInterpolation, 0, "compute Lennard-Jones potential using interpolation" },
      { "spline",       'P', 0, 'i', &cmd.spline,         0, "cubic-spline EAM tables in r^2 (thread_atom, cta_cell)" },
      { "usePairlist",  'L', 0, 'i', &cmd.usePairlist,    0, "pairlists for cta_cell LJ" },
      { "maxAtoms",      0,  1, 'i', &cmd.maxAtoms,       0, "link-cell slot capacity (0 = from the lattice)" },
      { "maxNeighbors",  0,  1, 'i', &cmd.maxNeighbors,   0, "neighbour-list rows per atom for *_nl (0 = from cutoff + skin)" },
      { "quiet",         0,  0, 'i', &cmd.quiet,          0, "no stdout report" },
      { "ljCutoffSigmas", 0, 1, 'd', &cmd.ljCutoffSigmas, 0, "LJ cutoff in sigmas (5 as in ljForce.c:114; 2.5 reproduces the cohesive energy of CoMD.c:897)" },
      { "deviceTimers",  0,  0, 'i', &cmd.deviceTimers,   0, "time the phases of timestep() with HIP events on the device (the host timers of the reference see launches, not kernels)" },
      { "pressure",      0,  0, 'i', &cmd.pressure,       0, "print the pressure (virial + kinetic, in GPa) at every printed step" },
      { "langevin",      0,  0, 'i', &cmd.langevin,       0, "BAOAB Langevin thermostat (NVT) in the integrator" },
      { "langevinTemp",  0,  1, 'd', &cmd.langevinTemp,   0, "Langevin target temperature (K; default: the -T value)" },
      { "langevinDamp",  0,  1, 'd', &cmd.langevinDamp,   0, "Langevin damping time tau (fs; default 100)" },
      { "seed",          0,  1, 'u', &cmd.seed,           0, "key of the Langevin noise (Philox4x32-10)" },
      { "rdf",           0,  1, 'i', &cmd.rdf,            0, "bins of the radial distribution function g(r), sampled at every printed step (0 = off, at most 4096)" },
      { "rdfMax",        0,  1, 'd', &cmd.rdfMax,         0, "range of g(r) in Angstroms (default and at most: the force cutoff)" },
      { "rdfFile",       0,  1, 's', cmd.rdfFile, sizeof cmd.rdfFile, "file g(r) is written to (default rdf.dat)" },
      { "msd",           0,  0, 'i', &cmd.msd,            0, "mean-squared displacement (unwrapped, tracked in the integrator), sampled at every printed step" },
      { "msdStart",      0,  1, 'i', &cmd.msdStart,       0, "global step the MSD origin is taken at (0..nSteps; default 0)" },
      { "msdFile",       0,  1, 's', cmd.msdFile, sizeof cmd.msdFile, "file the MSD is written to (default msd.dat)" },
      { "csp",           0,  0, 'i', &cmd.csp,            0, "centro-symmetry parameter and coordination number of every atom, sampled at every printed step (a Defects column)" },
      { "cspThreshold",  0,  1, 'd', &cmd.cspThreshold,   0, "an atom is a defect above this centro-symmetry parameter (Angstroms^2; default lat^2 / 4)" },
      { "cspCoord",      0,  1, 'd', &cmd.cspCoord,       0, "radius of the coordination count in Angstroms (default (1/sqrt 2 + 1) lat / 2; at most the force cutoff)" },
      { "cspFile",       0,  1, 's', cmd.cspFile, sizeof cmd.cspFile, "file the samples are written to (default csp.dat)" },
      { "cspDump",       0,  1, 's', cmd.cspDump, sizeof cmd.cspDump, "extended-XYZ file of the defect atoms of the last step (default: none)" },
      { "cna",           0,  0, 'i', &cmd.cna,            0, "adaptive common neighbour analysis (FCC / HCP / ICO / other per atom), sampled at every printed step (a NonFCC column)" },
      { "cnaFile",       0,  1, 's', cmd.cnaFile, sizeof cmd.cnaFile, "file the structure counts are written to (default cna.dat)" },
      { "cnaDump",       0,  1, 's', cmd.cnaDump, sizeof cmd.cnaDump, "extended-XYZ file of the non-FCC atoms of the last step (default: none)" },
      { "erateX",        0,  1, 'd', &cmd.erate[0],       0, "engineering strain rate of the box along x in 1/ps (1e9/s = 0.001; negative compresses; V/V0 and Sxx(GPa) columns)" },
      { "erateY",        0,  1, 'd', &cmd.erate[1],       0, "engineering strain rate of the box along y in 1/ps" },
      { "erateZ",        0,  1, 'd', &cmd.erate[2],       0, "engineering strain rate of the box along z in 1/ps" },
      { "deformStart",   0,  1, 'i', &cmd.deformStart,    0, "global step straining begins at (default 0)" },
      { "deformFile",    0,  1, 's', cmd.deformFile, sizeof cmd.deformFile, "file the stress-strain samples are written to (default deform.dat)" },
      { "stress",        0,  0, 'i', &cmd.stress,         0, "per-atom virial stress: hydrostatic pressure and von Mises stress, sampled at every printed step (a MaxVM(GPa) column)" },
      { "stressFile",    0,  1, 's', cmd.stressFile, sizeof cmd.stressFile, "file the samples are written to (default stress.dat)" },
      { "stressDump",    0,  1, 's', cmd.stressDump, sizeof cmd.stressDump, "extended-XYZ file of the per-atom stress tensors (GPa) of the last step (default: none)" },
      { "stressDumpMin", 0,  1, 'd', &cmd.stressDumpMin,  0, "only atoms with a von Mises stress of at least this many GPa are dumped (default 0: all atoms)" },
      { "strain",        0,  0, 'i', &cmd.strain,         0, "per-atom strain tensor, shear strain and D^2min against a reference snapshot, sampled at every printed step (a MaxShear column)" },
      { "strainRef",     0,  1, 'i', &cmd.strainRef,      0, "global step at whose end the reference is taken (0..nSteps; default 0)" },
      { "strainCutoff",  0,  1, 'd', &cmd.strainCutoff,   0, "neighbour radius of the strain fit in Angstroms (default (1/sqrt 2 + 1) lat / 2; at most the force cutoff)" },
      { "strainThreshold", 0, 1, 'd', &cmd.strainThreshold, 0, "atoms with a shear strain of at least this are counted (default 0.1)" },
      { "strainFile",    0,  1, 's', cmd.strainFile, sizeof cmd.strainFile, "file the samples are written to (default strain.dat)" },
      { "strainDump",    0,  1, 's', cmd.strainDump, sizeof cmd.strainDump, "extended-XYZ file of the per-atom strain tensors, shear strain and D^2min of the last step (default: none)" },
      { "strainDumpMin", 0,  1, 'd', &cmd.strainDumpMin,  0, "only atoms with a shear strain of at least this are dumped (default 0: all atoms)" },
      { "heatflux",      0,  0, 'i', &cmd.heatflux,       0, "heat flux and Green-Kubo thermal conductivity, sampled at every printed step (a Jx(eV/A^2/fs) column; -n sets the sampling interval)" },
      { "hfStart",       0,  1, 'i', &cmd.hfStart,        0, "global step the heat-flux sampling begins at (0..nSteps; default 0)" },
      { "hfWindow",      0,  1, 'i', &cmd.hfWindow,       0, "lags of the heat-flux autocorrelation (default 0: half the samples; clipped to the samples)" },
      { "hfFile",        0,  1, 's', cmd.hfFile, sizeof cmd.hfFile, "file the flux samples are written to (default heatflux.dat)" },
      { "hfAcfFile",     0,  1, 's', cmd.hfAcfFile, sizeof cmd.hfAcfFile, "file the autocorrelation and the running conductivity are written to (default hfacf.dat)" },
      { "baro",          0,  0, 'i', &cmd.baro,           0, "Berendsen barostat on a per-step pressure from the forces and the periodic face pairs (Pressure(GPa) and V/V0 columns; with --langevin: NPT)" },
      { "baroP",         0,  1, 'd', &cmd.baroP,          0, "barostat target pressure in GPa, compressive positive (default 0)" },
      { "baroTau",       0,  1, 'd', &cmd.baroTau,        0, "barostat coupling time in fs (default 1000)" },
      { "baroModulus",   0,  1, 'd', &cmd.baroModulus,    0, "bulk modulus the barostat assumes, in GPa (default 140)" },
      { "baroEvery",     0,  1, 'i', &cmd.baroEvery,      0, "steps between couplings (default 10)" },
      { "baroAxes",      0,  1, 's', cmd.baroAxes, sizeof cmd.baroAxes, "axes the barostat scales, a subset of xyz (default xyz; an axis with an --erate is not allowed)" },
      { "baroIso",       0,  0, 'i', &cmd.baroIso,        0, "one scale factor from the mean pressure of the chosen axes" },
      { "baroStart",     0,  1, 'i', &cmd.baroStart,      0, "global step coupling begins at (default 0)" },
      { "baroFile",      0,  1, 's', cmd.baroFile, sizeof cmd.baroFile, "file the couplings are written to (default baro.dat)" },
      { "profile",       0,  0, 'i', &cmd.profile,        0, "slab profiles along one axis (count, temperature, energies, mean velocity), sampled at every printed step" },
      { "profAxis",      0,  1, 's', cmd.profAxis, sizeof cmd.profAxis, "axis of the slabs: x, y or z (default x)" },
      { "profBins",      0,  1, 'i', &cmd.profBins,       0, "slabs along that axis, 1..1024 (default 20)" },
      { "profStart",     0,  1, 'i', &cmd.profStart,      0, "global step profile sampling begins at (default 0)" },
      { "profFile",      0,  1, 's', cmd.profFile, sizeof cmd.profFile, "file the time-averaged profile is written to (default profile.dat)" },
      { "mp",            0,  0, 'i', &cmd.mp,             0, "Mueller-Plathe momentum exchange between slab 0 (cold) and the middle slab (hot) of --profAxis / --profBins (turns --profile on; a dE(eV) column; thermal conductivity in the YAML)" },
      { "mpEvery",       0,  1, 'i', &cmd.mpEvery,        0, "steps between exchanges (default 100)" },
      { "mpSwaps",       0,  1, 'i', &cmd.mpSwaps,        0, "pairs of atoms an exchange swaps at most, 1..64 (default 1)" },
      { "mpStart",       0,  1, 'i', &cmd.mpStart,        0, "global step exchanging begins at (default 0)" },
      { "mpFile",        0,  1, 's', cmd.mpFile, sizeof cmd.mpFile, "file the exchanges are written to (default mp.dat)" },
      { "sk",            0,  1, 'i', &cmd.sk,             0, "static structure factor S(k) on the wave vectors 2 pi (sx h / Lx, sy k / Ly, sz l / Lz), h in 0..M, k, l in -M..M, M = 1..64 (0 = off), and the Bragg order, sampled at every printed step (an S111/N column)" },
      { "skStride",      0,  1, 's', cmd.skStride, sizeof cmd.skStride, "strides of the wave-vector grid, s or sx,sy,sz, each >= 1 with stride * M <= 65536 (default 1; -x,-y,-z gives the reciprocal lattice of the cubic cell)" },
      { "skBins",        0,  1, 'i', &cmd.skBins,         0, "|k| bins of the powder average, 1..4096 (default 50)" },
      { "skStart",       0,  1, 'i', &cmd.skStart,        0, "global step structure-factor sampling begins at (0..nSteps; default 0)" },
      { "skFile",        0,  1, 's', cmd.skFile, sizeof cmd.skFile, "file the time-averaged powder average S(|k|) is written to (default sk.dat)" },
      { "steinhardt",    0,  0, 'i', &cmd.steinhardt,     0, "Steinhardt bond-orientational order q4, q6, w4, w6 of every atom on its 12 nearest neighbours, sampled at every printed step (a MeanQ6 column)" },
      { "stSolid",       0,  1, 'd', &cmd.stSolid,        0, "atoms with q6 of at least this count as solid-like, 0 < x < 1 (default 0.45)" },
      { "stFile",        0,  1, 's', cmd.stFile, sizeof cmd.stFile, "file the samples are written to (default steinhardt.dat)" },
      { "stDump",        0,  1, 's', cmd.stDump, sizeof cmd.stDump, "extended-XYZ file of q4, q6, w4, w6 of the atoms of the last step (default: none)" },
      { "stDumpMax",     0,  1, 'd', &cmd.stDumpMax,      0, "only atoms with q6 of at most this are dumped, and the atoms with fewer than 12 neighbours (default inf: all atoms)" },
      { "elastic",       0,  0, 'i', &cmd.elastic,        0, "Born matrix at every printed step and the stress-fluctuation elastic constants C11, C12, C44, K, G at the end of the run (a C11B(GPa) column; a fixed box: not with --erateX/Y/Z or --baro)" },
      { "elStart",       0,  1, 'i', &cmd.elStart,        0, "global step elastic sampling begins at (0..nSteps; default 0)" },
      { "elFile",        0,  1, 's', cmd.elFile, sizeof cmd.elFile, "file the samples and the elastic constants are written to (default elastic.dat)" },
   };
   const int nDefs = (int)(sizeof defs / sizeof defs[0]);

   struct option* longOpts = (struct option*)calloc((size_t)nDefs + 1, sizeof(struct option));
   char shortOpts[4 * 32]; int so = 0;
   for (int i = 0; i < nDefs; ++i) {
      longOpts[i].name = defs[i].longName;
      longOpts[i].has_arg = defs[i].hasArg ? required_argument : no_argument;
      longOpts[i].flag = NULL;
      longOpts[i].val = defs[i].shortName ? defs[i].shortName : 1000 + i;
      if (defs[i].shortName) { shortOpts[so++] = defs[i].shortName; if (defs[i].hasArg) shortOpts[so++] = ':'; }
   }
   shortOpts[so] = '\0';

   optind = 1;            /* allow repeated parsing inside one process (library use) */
   int c, idx;
   while ((c = getopt_long(argc, argv, shortOpts, longOpts, &idx)) != -1) {
      const ArgDef* d = NULL;
      for (int i = 0; i < nDefs; ++i) if (longOpts[i].val == c) { d = &defs[i]; break; }
      if (!d) { fprintf(screenOut, "\n\n    invalid switch : -%c in getopt()\n\n\n", optopt); continue; }
      if (!d->hasArg) { *(int*)d->ptr = 1; continue; }
      switch (d->type) {
         case 'i': *(int*)d->ptr = atoi(optarg); break;
         case 'd': *(double*)d->ptr = atof(optarg);
                   if (d->ptr == &cmd.cspThreshold) cmd.cspThresholdSet = 1;
                   if (d->ptr == &cmd.cspCoord) cmd.cspCoordSet = 1;
                   if (d->ptr == &cmd.strainCutoff) cmd.strainCutoffSet = 1;
                   break;
         case 'u': *(uint64_t*)d->ptr = strtoull(optarg, NULL, 0); break;
         case 's': strncpy((char*)d->ptr, optarg, (size_t)d->size - 1); ((char*)d->ptr)[d->size - 1] = '\0'; break;
      }
   }
   free(longOpts);

   if (strlen(cmd.potName) == 0) {
      if (strcmp(cmd.potType, "setfl") == 0) strcpy(cmd.potName, "Cu01.eam.alloy");
      if (strcmp(cmd.potType, "funcfl") == 0) strcpy(cmd.potName, "Cu_u6.eam");
   }
   if (isnan(cmd.langevinTemp)) cmd.langevinTemp = cmd.temperature;
   if (help) { printArgs(defs, nDefs); exit(2); }
   return cmd;
}

void printCmdYaml(FILE* file, Command* cmd)
{
   if (!printRank() || !file) return;
   fprintf(file,
           "Command Line Parameters:\n"
           "  doeam: %d\n"
           "  potDir: %s\n"
           "  potName: %s\n"
           "  potType: %s\n"
           "  nx: %d\n"
           "  ny: %d\n"
           "  nz: %d\n"
           "  xproc: %d\n"
           "  yproc: %d\n"
           "  zproc: %d\n"
           "  Lattice constant: %g Angstroms\n"
           "  nSteps: %d\n"
           "  printRate: %d\n"
           "  Time step: %g fs\n"
           "  Initial Temperature: %g K\n"
           "  Initial Delta: %g Angstroms\n\n"
           "  GPU async opt: %d\n"
           "  GPU profiling mode: %d\n"
           "  GPU method: %s\n"
           "  Space-filling (Hilbert): %d\n",
           cmd->doeam, cmd->potDir, cmd->potName, cmd->potType, cmd->nx, cmd->ny, cmd->nz,
           cmd->xproc, cmd->yproc, cmd->zproc, cmd->lat, cmd->nSteps, cmd->printRate, cmd->dt,
           cmd->temperature, cmd->initialDelta, cmd->gpuAsync, cmd->gpuProfile, cmd->method, cmd->doHilbert);
   if (cmd->langevin)
      fprintf(file,
              "  Langevin thermostat: 1\n"
              "  Langevin temperature: %g K\n"
              "  Langevin damping: %g fs\n"
              "  Langevin seed: %llu\n",
              cmd->langevinTemp, cmd->langevinDamp, (unsigned long long)cmd->seed);
   if (cmd->csp) fprintf(file, "  CSP file: %s\n", cmd->cspFile);
   if (cmd->cna) fprintf(file, "  CNA file: %s\n", cmd->cnaFile);
   if (cmd->stress) fprintf(file, "  Stress file: %s\n", cmd->stressFile);
   if (cmd->strain) fprintf(file, "  Strain reference step: %d\n  Strain file: %s\n", cmd->strainRef, cmd->strainFile);
   if (cmd->heatflux) fprintf(file, "  Heat flux from step: %d\n  Heat flux file: %s\n  Heat flux ACF file: %s\n", cmd->hfStart, cmd->hfFile, cmd->hfAcfFile);
   if (cmd->msd) fprintf(file, "  MSD from step: %d\n  MSD file: %s\n", cmd->msdStart, cmd->msdFile);
   if (cmd->erate[0] != 0.0 || cmd->erate[1] != 0.0 || cmd->erate[2] != 0.0)
      fprintf(file, "  Strain rates: [ %g, %g, %g ] 1/ps\n  Deform from step: %d\n  Deform file: %s\n", cmd->erate[0], cmd->erate[1], cmd->erate[2], cmd->deformStart, cmd->deformFile);
   if (cmd->baro)
      fprintf(file, "  Barostat: 1\n  Barostat target: %g GPa\n  Barostat tau: %g fs\n  Barostat modulus: %g GPa\n  Barostat every: %d steps\n  Barostat axes: %s%s\n  Barostat from step: %d\n"
                    "  Barostat file: %s\n", cmd->baroP, cmd->baroTau, cmd->baroModulus, cmd->baroEvery, cmd->baroAxes, cmd->baroIso ? " (iso)" : "", cmd->baroStart, cmd->baroFile);
   if (cmd->profile || cmd->mp)
      fprintf(file, "  Profile axis: %s\n  Profile bins: %d\n  Profile from step: %d\n  Profile file: %s\n", cmd->profAxis, cmd->profBins, cmd->profStart, cmd->profFile);
   if (cmd->mp)
      fprintf(file, "  MullerPlathe every: %d steps\n  MullerPlathe swaps: %d\n  MullerPlathe from step: %d\n  MullerPlathe file: %s\n", cmd->mpEvery, cmd->mpSwaps, cmd->mpStart, cmd->mpFile);
   if (cmd->sk) fprintf(file, "  Structure factor kMax index: %d\n  Structure factor stride: %s\n  Structure factor bins: %d\n  Structure factor from step: %d\n  Structure factor file: %s\n",
                        cmd->sk, cmd->skStride, cmd->skBins, cmd->skStart, cmd->skFile);
   if (cmd->steinhardt) fprintf(file, "  Steinhardt solid threshold: %g\n  Steinhardt file: %s\n", cmd->stSolid, cmd->stFile);
   if (cmd->elastic) fprintf(file, "  Elastic from step: %d\n  Elastic file: %s\n", cmd->elStart, cmd->elFile);
   fprintf(file, "\n");
   fflush(file);
}
