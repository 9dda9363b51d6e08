/* comd_host.h -- host side (plain C11) of the MI355X CoMD hot path.
 *
 * Mirrors the reference's operator surface so the loop reads like src-mpi/timestep.c:
 *   BasePotential {force, print, destroy}      CoMDTypes.h:42-53
 *   HaloExchange  {loadBuffer, unloadBuffer, destroy}   haloExchange.h:84-104
 *   timestep(), computeForce(), redistributeAtoms(), kineticEnergyGpu()   timestep.c:48-276
 * and calls the device only through include/comd_hip.h.  No HIP headers here.
 */
#ifndef COMD_HOST_H
#define COMD_HOST_H

#include <stdio.h>
#include <stdint.h>
#include "comd_hip.h"
#include "comd_geometry.h"

#define screenOut stdout

/* mytype.h:10-19: scanf format of a real_t */
#ifdef COMD_SINGLE
#define FMT1 "%g"
#else
#define FMT1 "%lg"
#endif

/* ---- constants.h:14-39 ---- */
#define amuInKilograms  1.660538921e-27
#define fsInSeconds     1.0e-15
#define AngsInMeters    1.0e-10
#define eVInJoules      1.602176565e-19
static const double amuToInternalMass = amuInKilograms * AngsInMeters * AngsInMeters / (fsInSeconds * fsInSeconds * eVInJoules);
static const double kB_eV = 8.6173324e-5;
static const double hartreeToEv = 27.21138505;
static const double bohrToAngs = 0.52917721092;

/* ---- command line: mycommand.h ---- */
typedef struct CommandSt {
   char potDir[1024], potName[1024], potType[1024], method[1024];
   int doeam, nx, ny, nz, xproc, yproc, zproc, nSteps, printRate;
   double dt, lat, temperature, initialDelta, relativeSkinDistance;
   int doHilbert, gpuAsync, gpuProfile, ljInterpolation, spline, usePairlist, maxNeighbors;
   int maxAtoms;          /* extension: link-cell slot capacity, 0 = choose from the lattice (reference: -DMAXATOMS) */
   int quiet;             /* extension: suppress the stdout report (library use) */
   int deviceTimers;      /* extension: HIP-event timing of the phases of timestep() (the reference's host timers are not device-synchronised) */
   double ljCutoffSigmas; /* extension (tests): LJ cutoff in sigmas; 5 = the reference (ljForce.c:114), 2.5 = upstream CoMD, whose cohesive energy CoMD.c:897 documents */
   int pressure;          /* extension: pressure column in the report (virial + kinetic tensor at every printed step, the reference has none) */
   int langevin;          /* extension: BAOAB Langevin thermostat (NVT) in the integrator; the reference integrates NVE only */
   double langevinTemp;   /* extension: its target in K; NAN until given = the -T value */
   double langevinDamp;   /* extension: its damping time tau in fs (default 100) */
   uint64_t seed;         /* extension: the key of its Philox noise (default COMD_LANGEVIN_SEED) */
   int rdf;               /* extension: bins of the radial distribution function sampled at every printed step, 0 = off (the reference has no structural analysis) */
   double rdfMax;         /* extension: its range in Angstroms; <= 0 = the force cutoff */
   char rdfFile[1024];    /* extension: where the print rank writes it (default rdf.dat) */
   int msd;               /* extension: mean-squared displacement from displacements tracked in the drift kernels, sampled at every printed step (the reference has no dynamical analysis) */
   int msdStart;          /* extension: the global step its origin is taken at, 0..nSteps (default 0) */
   char msdFile[1024];    /* extension: where the print rank writes it (default msd.dat) */
   int csp;               /* extension: centro-symmetry parameter and coordination number of every atom, sampled at every printed step (the reference has no structural analysis) */
   double cspThreshold;   /* extension: an atom is a defect when its parameter exceeds this, in Angstroms^2; 0 = lat^2 / 4 */
   double cspCoord;       /* extension: radius of the coordination count in Angstroms; 0 = halfway between the first two FCC shells */
   char cspFile[1024];    /* extension: where the print rank writes the samples (default csp.dat) */
   char cspDump[1024];    /* extension: extended-XYZ file of the defect atoms of the last step; empty = none */
   int cspThresholdSet, cspCoordSet;   /* the two values were given (a given 0 is refused, an absent one means the default) */
   int cna;               /* extension: adaptive common neighbour analysis, FCC / HCP / ICO / other per atom, sampled at every printed step */
   char cnaFile[1024];    /* extension: where the print rank writes the samples (default cna.dat) */
   char cnaDump[1024];    /* extension: extended-XYZ file of the non-FCC atoms of the last step; empty = none */
   double erate[3];       /* extension: engineering strain rates of the box along x, y, z in 1/ps (1e9/s = 0.001), negative compresses; all 0 = a fixed box, as in the reference */
   int deformStart;       /* extension: the global step straining begins at (default 0) */
   char deformFile[1024]; /* extension: where the print rank writes the stress-strain samples (default deform.dat) */
   int stress;            /* extension: per-atom virial stress, its hydrostatic pressure and von Mises stress reduced on the device at every printed step */
   char stressFile[1024]; /* extension: where the print rank writes the samples (default stress.dat) */
   char stressDump[1024]; /* extension: extended-XYZ file of the per-atom tensors of the last step; empty = none */
   double stressDumpMin;  /* extension: only atoms with a von Mises stress of at least this many GPa are dumped; 0 = all */
   int strain;            /* extension: per-atom strain tensor, shear strain and D^2min against a reference snapshot, reduced on the device at every printed step */
   int strainRef;         /* extension: the global step the reference is taken at, 0..nSteps (default 0) */
   double strainCutoff;   /* extension: the neighbour radius r_s in Angstroms; absent = that of --cspCoord, halfway between the first two FCC shells */
   int strainCutoffSet;   /* the value was given (a given 0 is refused, an absent one means the default) */
   double strainThreshold;/* extension: atoms with a shear strain of at least this are counted (default 0.1) */
   char strainFile[1024]; /* extension: where the print rank writes the samples (default strain.dat) */
   char strainDump[1024]; /* extension: extended-XYZ file of the per-atom tensors of the last step; empty = none */
   double strainDumpMin;  /* extension: only atoms with a shear strain of at least this are dumped; 0 = all */
   int heatflux;          /* extension: the heat flux J V, reduced on the device at every printed step, its autocorrelation and the Green-Kubo thermal conductivity */
   int hfStart;           /* extension: the global step sampling begins at, 0..nSteps (default 0) */
   int hfWindow;          /* extension: lags of the autocorrelation; 0 = half the samples; more than the samples is clipped */
   char hfFile[1024];     /* extension: where the print rank writes the flux samples (default heatflux.dat) */
   char hfAcfFile[1024];  /* extension: where it writes the autocorrelation and the running conductivity (default hfacf.dat) */
   int baro;              /* extension: Berendsen barostat on the pressure of comdVirialFdotr; the reference's box is fixed */
   double baroP;          /* extension: its target pressure in GPa, compressive positive (default 0) */
   double baroTau;        /* extension: its coupling time in fs (default 1000) */
   double baroModulus;    /* extension: the bulk modulus the scale rule assumes, in GPa (default 140) */
   int baroEvery;         /* extension: steps between couplings (default 10) */
   char baroAxes[16];     /* extension: the axes it scales, a subset of xyz (default xyz) */
   int baroIso;           /* extension: one scale factor from the mean pressure of the chosen axes */
   int baroStart;         /* extension: the global step coupling begins at (default 0) */
   char baroFile[1024];   /* extension: where the print rank writes the couplings (default baro.dat) */
   int profile;           /* extension: slab profiles of count, temperature, energy and velocity along one axis, sampled at the printed steps */
   char profAxis[16];     /* extension: the axis of the slabs, x, y or z (default x) */
   int profBins;          /* extension: slabs along that axis, 1..1024 (default 20) */
   int profStart;         /* extension: the global step sampling begins at (default 0) */
   char profFile[1024];   /* extension: where the print rank writes the time-averaged profile (default profile.dat) */
   int mp;                /* extension: Mueller-Plathe momentum exchange between slab 0 and slab profBins / 2; turns --profile on */
   int mpEvery;           /* extension: steps between exchanges (default 100) */
   int mpSwaps;           /* extension: pairs of atoms an exchange swaps at most, 1..64 (default 1) */
   int mpStart;           /* extension: the global step exchanging begins at (default 0) */
   char mpFile[1024];     /* extension: where the print rank writes the exchanges (default mp.dat) */
   int sk;                /* extension: the static structure factor on the half grid h in [0, M], k, l in [-M, M] and the Bragg order, sampled at the printed steps; M, 0 = off */
   char skStride[64];     /* extension: the strides of the grid, s or sx,sy,sz (default 1) */
   int skBins;            /* extension: |k| bins of the powder average, 1..4096 (default 50) */
   int skStart;           /* extension: the global step sampling begins at (default 0) */
   char skFile[1024];     /* extension: where the print rank writes the time-averaged powder average (default sk.dat) */
   int steinhardt;        /* extension: Steinhardt's bond-orientational order q4, q6, w4, w6 of every atom, reduced on the device at every printed step */
   double stSolid;        /* extension: atoms with q6 of at least this are counted as solid-like, 0 < x < 1 (default 0.45) */
   char stFile[1024];     /* extension: where the print rank writes the samples (default steinhardt.dat) */
   char stDump[1024];     /* extension: extended-XYZ file of the per-atom values of the last step; empty = none */
   double stDumpMax;      /* extension: only atoms with q6 of at most this are dumped, the invalid ones always; +inf = all */
   int elastic;           /* extension: the Born matrix at every printed step, and the stress-fluctuation elastic constants at the end of the run */
   int elStart;           /* extension: the global step sampling begins at (0..nSteps; default 0) */
   char elFile[1024];     /* extension: where the print rank writes the samples and the constants (default elastic.dat) */
} Command;

#define COMD_LANGEVIN_SEED 0x436f4d44ull     /* "CoMD" */
#define COMD_LANGEVIN_DAMP 100.0

Command parseCommandLine(int argc, char** argv);
void printCmdYaml(FILE* file, Command* cmd);

/* ---- parallel layer: parallel.h.  One process per GPU; the transport is pluggable. ---- */
/* CommTransport: include/comd_hip.h */

void initParallel(int rank, int nRanks, const CommTransport* transport);   /* parallel.c:57-64 */
void destroyParallel(void);
int  loopbackParallel(void);
int  getNRanks(void);
int  getMyRank(void);
int  printRank(void);
void barrierParallel(void);
void timestampBarrier(const char* msg);
int  sendReceiveParallel(void* sendBuf, int sendLen, int dest, void* recvBuf, int recvLen, int source);
int  sendReceiveDevice(void* sendBuf, int sendLen, int dest, void* recvBuf, int recvLen, int source, comdStream_t stream);
void sendReceiveDevice2(void* sendM, int nSendM, int dstM, void* recvP, void* sendP, int nSendP, int dstP, void* recvM,
                        int recvCap, comdStream_t stream, int nRecv[2]);
int  sizedExchangeAvailable(void);
void sendReceiveDevice2Sized(void* sendM, int nSendM, int dstM, void* recvP, int nRecvP, void* sendP, int nSendP, int dstP, void* recvM, int nRecvM,
                             comdStream_t stream);
void addIntParallel(int* sendBuf, int* recvBuf, int count);
void addRealParallel(real_t* sendBuf, real_t* recvBuf, int count);
void addDoubleParallel(double* sendBuf, double* recvBuf, int count);
void addIntParallelLong(int* sendBuf, int* recvBuf, size_t count);            /* counts beyond an int: in chunks of 2^28 */
void addDoubleParallelLong(double* sendBuf, double* recvBuf, size_t count);
void maxIntParallel(int* sendBuf, int* recvBuf, int count);
void bcastParallel(void* buf, int len, int root);

/* ---- decomposition.h ---- */
typedef struct DomainSt {
   int procGrid[3], procCoord[3];
   real_t globalMin[3], globalMax[3], globalExtent[3];
   real_t localMin[3], localMax[3], localExtent[3];
} Domain;
Domain* initDecomposition(int xproc, int yproc, int zproc, const real_t globalExtent[3]);
void setDomainExtent(Domain* domain, const real_t globalExtent[3]);    /* global and local extents of a decomposition: initDecomposition and comdSetBox */
int processorNum(Domain* domain, int dix, int diy, int diz);

/* ---- linkCells.h ---- */
typedef struct LinkCellSt {
   int gridSize[3];
   int nLocalBoxes, nHaloBoxes, nTotalBoxes;
   real_t localMin[3], localMax[3], boxSize[3], invBoxSize[3];
   int* nAtoms;           /* host copy; refreshed from the device by sumAtoms */
   int maxAtoms;          /* slot capacity per cell */
   int *boxIDLookUp, *boxIDLookUpReverse;   /* -H: Hilbert numbering of the local cells (linkCells.h:27-28); NULL otherwise */
   CellGeom geom;
   real_t builtRange;     /* the interaction range the grid was sized for (cutoff, + skin for the *_nl methods): no cell may become narrower (comdSetBox) */
} LinkCell;
LinkCell* initLinkCells(const Domain* domain, real_t cutoff, int useHilbert);
void setLinkCellExtent(LinkCell* boxes, const Domain* domain);          /* bounds, cell widths and geom of the same grid over the domain as it is now */
void destroyLinkCells(LinkCell** boxes);
int getNeighborBoxes(LinkCell* boxes, int iBox, int* nbrBoxes);
int getBoxFromTuple(LinkCell* boxes, int x, int y, int z);
int getBoxFromCoord(LinkCell* boxes, const real_t rr[3]);
int maxOccupancy(LinkCell* boxes);

/* ---- initAtoms.h ---- */
typedef struct AtomsSt {
   int nLocal, nGlobal;
   HostAtoms h;           /* slot arrays, cell*maxAtoms + i */
} Atoms;
struct SimFlatSt;
Atoms* initAtoms(LinkCell* boxes);
void destroyAtoms(Atoms* atoms);
/* pass 1 (atoms == NULL storage): returns the largest per-cell count the lattice produces on this rank */
int  countFccLattice(int nx, int ny, int nz, real_t lat, const Domain* domain, LinkCell* boxes);
void createFccLattice(int nx, int ny, int nz, real_t lat, struct SimFlatSt* s);
void setTemperature(struct SimFlatSt* s, real_t temperature);
void randomDisplacements(struct SimFlatSt* s, real_t delta);
int  putAtomInBox(LinkCell* boxes, Atoms* atoms, int gid, int iType, real_t x, real_t y, real_t z, real_t px, real_t py, real_t pz);
void kineticEnergyHost(struct SimFlatSt* s);   /* timestep.c:109-133, used during initialisation only */

/* ---- random.h ---- */
real_t   gasdev(uint64_t* seed);
double   lcg61(uint64_t* seed);
uint64_t mkSeed(uint32_t id, uint32_t callSite);

/* ---- potentials: CoMDTypes.h:42-53, 140-201 ---- */
typedef struct BasePotentialSt {
   real_t cutoff, mass, lat;
   char latticeType[8];
   char name[3];
   int atomicNo;
   int  (*force)(struct SimFlatSt* s);
   void (*print)(FILE* file, struct BasePotentialSt* pot);
   void (*destroy)(struct BasePotentialSt** pot);
} BasePotential;

typedef struct LjPotentialSt {
   real_t cutoff, mass, lat; char latticeType[8]; char name[3]; int atomicNo;
   int  (*force)(struct SimFlatSt* s);
   void (*print)(FILE* file, BasePotential* pot);
   void (*destroy)(BasePotential** pot);
   real_t sigma, epsilon;
} LjPotential;

typedef struct InterpolationObjectSt {
   int n; real_t x0, invDx; real_t* values; real_t invDxXx0;
} InterpolationObject;

struct HaloExchangeSt;
typedef struct EamPotentialSt {
   real_t cutoff, mass, lat; char latticeType[8]; char name[3]; int atomicNo;
   int  (*force)(struct SimFlatSt* s);
   void (*print)(FILE* file, BasePotential* pot);
   void (*destroy)(BasePotential** pot);
   InterpolationObject *phi, *rho, *f;
   real_t *phiSpline, *rhoSpline;     /* -P: 4 * n cubic-spline coefficients in r^2 each (gpu_utility.c:377-430), else NULL */
   struct HaloExchangeSt* forceExchange;
} EamPotential;

BasePotential* initLjPot(void);
BasePotential* initEamPot(const char* dir, const char* file, const char* type);
void interpolate(InterpolationObject* table, real_t r, real_t* f, real_t* df);
real_t* initSplineCoefficients(int n, const real_t* values, real_t x0, real_t invDx);   /* malloc'd, 4 * n */
void eamUseSplines(BasePotential* pot);                                                /* fill phiSpline / rhoSpline */

typedef struct SpeciesDataSt { char name[3]; int atomicNo; real_t mass; } SpeciesData;
typedef struct ValidateSt { double eTot0; int nAtoms0; } Validate;

/* ---- halo exchange: haloExchange.h ---- */
enum HaloFaceOrder { HALO_X_MINUS, HALO_X_PLUS, HALO_Y_MINUS, HALO_Y_PLUS, HALO_Z_MINUS, HALO_Z_PLUS };
enum HaloAxisOrder { HALO_X_AXIS, HALO_Y_AXIS, HALO_Z_AXIS };

/* Per axis: the counts (atoms) of the four messages of the previous exchange -- sent through the minus face, sent through the plus face,
 * received from the plus neighbour, received from the minus neighbour -- mirrored by a one-wave kernel into pinned memory.  Sender and
 * receiver of a message hold the same number, so both size the next transfer as count + 12.5 % + 64 without talking to each other. */
typedef struct HaloSpecSt {
   int   valid;                           /* mirror[] describes the previous exchange of this axis */
   int   pending;                         /* the mirror kernel has been enqueued: wait for `event` before reading */
   int*  mirror;                          /* pinned [4] */
   void* event;
   int   haveBound, lastBound[4];         /* sizes the previous exchange was posted with: a count above its bound means that exchange was cut short */
   int   lastCount[4];                    /* ... and the counts those sizes were derived from (both ends of a message hold the same two numbers) */
} HaloSpec;

enum HaloKind { HALO_ATOMS, HALO_FORCE, HALO_POSITIONS };      /* whole atoms; dF/drho, 1 real per atom; positions + face shift, 3 reals per atom */

typedef struct HaloExchangeSt {
   int nbrRank[6];
   int bufCapacity;                       /* bytes per message buffer */
   /* the device exchanges: both faces of an axis phase packed / unpacked by one device launch each.  nBytes -1: "ask msgBytes2 when you need it" */
   void (*loadBuffer2)(struct HaloExchangeSt* hh, void* data, int faceM, char* bufM, int faceP, char* bufP, int nBytes[2]);
   void (*unloadBuffer2)(struct HaloExchangeSt* hh, void* data, int faceA, int bufSizeA, char* bufA, int faceB, int bufSizeB, char* bufB);
   /* sizes of the two packed device messages of an axis phase, behind one synchronisation at the most */
   void (*msgBytes2)(struct HaloExchangeSt* hh, void* data, int faceM, char* bufM, int faceP, char* bufP, int out[2]);
   /* the reference's one-face plugin shape, used where loadBuffer2 / unloadBuffer2 are NULL: comdHaloExchangeHost fills them with its caller's host callbacks */
   int (*loadBuffer)(void* parms, void* data, int face, char* buf);       /* returns bytes */
   void (*unloadBuffer)(void* parms, void* data, int face, int bufSize, char* buf);
   void (*destroy)(void* parms);
   void* parms;
   enum HaloKind kind;
   int deviceBuffers;                     /* 1: the four buffers are device memory */
   char *sendBufM, *sendBufP, *recvBufM, *recvBufP;
   /* size agreement without a handshake (device buffers, messages that leave the rank) */
   int msgHeaderBytes, msgBytesPerAtom;   /* bytes of a message of n atoms = msgHeaderBytes + n * msgBytesPerAtom */
   int capacityAtoms;
   int exactCounts;                       /* counts cannot change between invalidations (positions between list builds): no slack */
   /* optional: device addresses of the four counts of axis phase (faceM, faceP), in HaloSpec order */
   void (*countPtrs)(void* parms, struct HaloExchangeSt* hh, int faceM, int faceP, const int* out[4]);
   /* optional: tell the plugin the agreed sizes (atoms) of the message it packs for `face` and of the one it unpacks for `face`; 0 = none */
   void (*setBounds)(void* parms, int face, int sendBoundAtoms, int recvBoundAtoms);
   HaloSpec spec[3];
   /* optional: fill the halo cells of axes firstAxis..2 (all of them self-neighbour axes) straight from their sources, one launch (comd_hip.h mirrorSlotCellsGpu) */
   void (*mirror)(struct HaloExchangeSt* hh, void* data, int firstAxis);
   int nTotalBoxes;                       /* (for the mirror map) */
} HaloExchange;

typedef struct AtomExchangeParmsSt {
   int nCells[6];
   int* cellList[6];                      /* host */
   int* cellListGpu[6];                   /* device */
   int* d_cellOffsets;                    /* device scratch, max nCells + 1 */
   int* d_cellOffsets2;                   /* second scratch: the two faces of an axis phase are scanned and packed together */
   real_t shift[6][3];                    /* pbcFactor * globalExtent */
   int capacityAtoms;
   int sendBound[6], recvBound[6];        /* agreed message sizes in atoms, 0 = none (capacityAtoms applies) */
} AtomExchangeParms;

typedef struct ForceExchangeParmsSt {
   int nCells[6];
   int *sendCells[6], *recvCells[6];
   int *sendCellsGpu[6], *recvCellsGpu[6];
   int *sendOffsetsGpu[6], *recvOffsetsGpu[6];   /* device, nCells + 1 each: filled by one batched scan per step */
   int capacityAtoms;
   /* mirror map of the self-neighbour tail firstAxis..2 (built on first use): halo cell mirrorDst[k] is the image of mirrorSrc[k] displaced by mirrorShift[3k..] */
   int mirrorFirst, mirrorPairs;
   int *mirrorDstGpu, *mirrorSrcGpu; real_t* mirrorShiftGpu;
   int mirrorStale;                       /* haloSetBox: shift[][] has changed since mirrorShiftGpu was filled */
   real_t shift[6][3];
   int msgBytesCached[6];                 /* message sizes of the last blocking read; positions: fixed between list builds, so kept; -1 = unknown */
   int sendBound[6];                      /* agreed message sizes in atoms, 0 = none */
} ForceExchangeParms;

HaloExchange* initAtomHaloExchange(Domain* domain, LinkCell* boxes, int allocDevice);
HaloExchange* initForceHaloExchange(Domain* domain, LinkCell* boxes, int allocDevice);
/* Verlet-list mode: refresh of the halo copies' positions between list builds, over the force exchange's cell lists */
HaloExchange* initPositionHaloExchange(Domain* domain, LinkCell* boxes, int allocDevice);
void preparePositionExchange(HaloExchange* positionExchange, struct SimFlatSt* sim);   /* after every list build */
void haloSetBox(HaloExchange* haloExchange, const Domain* domain);                     /* the periodic shifts (and the mirror path's table of them) after comdSetBox */
void destroyHaloExchange(HaloExchange** haloExchange);
void invalidateHaloSizes(HaloExchange* haloExchange);      /* the next exchange of every axis swaps exact sizes again */
void haloExchange(HaloExchange* haloExchange, void* data);
void comdSetHaloHandshake(int on);                          /* 1: swap exact message sizes before every exchange (COMD_HALO_HANDSHAKE=1), 0: sized protocol, -1: ask the environment */
int  haloMirrorFirstAxis(const HaloExchange* hh);         /* first axis of the self-neighbour tail the plugin mirrors directly; 3 = none */
void exchangeData(HaloExchange* haloExchange, void* data, int iAxis);
void prepareForceExchange(HaloExchange* forceExchange, struct SimFlatSt* sim);   /* one batched scan of all twelve cell lists */
int* mkAtomCellList(LinkCell* boxes, enum HaloFaceOrder iFace, int nCells);
int* mkForceSendCellList(LinkCell* boxes, int face, int nCells);
int* mkForceRecvCellList(LinkCell* boxes, int face, int nCells);

/* a table of samples that grows by doubling (the reports keep one row per sample, the barostat and the exchange one per event): n rows of the width its owner gives nextRow */
typedef struct RowTableSt { void* rows; int n, cap; } RowTable;
void* nextRow(RowTable* t, size_t rowBytes);      /* the next row, rowBytes wide: the table grows as needed (reports.c) */

/* ---- simulation: CoMDTypes.h:75-135 ---- */
typedef struct SimFlatSt {
   int nSteps, printRate;
   double dt;
   Domain* domain;
   LinkCell* boxes;
   Atoms* atoms;
   SpeciesData* species;
   real_t ePotential, eKinetic;
   BasePotential* pot;
   HaloExchange* atomExchange;
   HaloExchange* positionExchange;  /* *_nl methods only */
   SimGpu gpu;
   int method;
   int n_boundary_cells, n_boundary1_cells;
   int *boundary_cells_h, *interior_cells_h, *boundary1_cells_h;
   int gpuAsync, gpuProfile;
   int ljInterpolation, spline, usePairlist;
   real_t* ljTable;                 /* -I: the table of comdLjInterpolationTable (ljTableN + 4 entries), NULL otherwise */
   int ljTableN;
   real_t ljTableX0, ljTableInvDx;
   real_t skinDistance;
   int useNL;                       /* method is thread_atom_nl / warp_atom_nl */
   int interiorLaunched;            /* -a 1: redistributeAtoms has already started the interior cells' force work */
   int nlBuilds;                    /* list builds so far (reported) */
   int quiet, cmdDoeam;
   int iStepPrev, firstPrint;       /* printThings state (static locals in CoMD.c:466-467) */
   int pressure;                    /* --pressure: the Pressure(GPa) column of printThings and the YAML block, from what computePressure left in W, K, V */
   real_t W[6], K[6], V;            /* computePressure: global pair virial and kinetic tensor in eV (xx yy zz yz xz xy), volume in A^3 */
   int langevin;                    /* --langevin / comdSetLangevin: timestep() runs the BAOAB Langevin kernels */
   double langevinTemp, langevinDamp;   /* target (K) and damping time tau (fs) */
   uint64_t langevinSeed;           /* Philox key */
   uint64_t stepCount;              /* global step index: 0 at creation, one per step of timestep(), the same on every rank (the noise counter) */
   int rdfBins;                     /* --rdf: comdMain samples the pair histogram at every printed step; 0 = off */
   double rdfMax;                   /* its range in Angstroms (the force cutoff unless --rdfMax) */
   char rdfFile[1024];
   double* rdfSum;                  /* [rdfBins] global unordered pair counts summed over the samples */
   int rdfSamples;
   int trackDisp;                   /* comdTrackDisplacement: the drift kernels add every atom's motion into the device records of its gid */
   int msd, msdStart;               /* --msd: comdMain tracks from global step msdStart on and samples the MSD at every printed step */
   char msdFile[1024];
   RowTable msdRows;                /* [8] doubles: step, the seven values of comdMsd */
   double msdNow;                   /* the MSD(A^2) column of printThings: the last sample, 0 before the origin */
   double lat;                      /* the lattice constant the crystal was made with (-l, or the potential's) */
   int csp;                         /* --csp: comdMain samples the centro-symmetry parameter at every printed step */
   double cspThreshold, cspCoord;   /* defect threshold (A^2) and coordination radius (A), defaults resolved */
   char cspFile[1024], cspDump[1024];
   RowTable cspRows;                /* [7] doubles: step, defects, atoms with fewer than 12 neighbours, mean and max of the finite csp, mean coordination, atoms with coordination != 12 */
   double* cspLast;                 /* [2 nGlobal]: csp and coordination by gid of the last sample (--cspDump) */
   void* analysisStage;             /* the by-gid analyses (analysis.c): host staging for the by-slot results, the gids and the occupancies, kept between calls */
   size_t analysisStageBytes;
   int cspDefectsNow;               /* the Defects column of printThings: the last sample */
   int cna;                         /* --cna: comdMain samples the structure types at every printed step */
   char cnaFile[1024], cnaDump[1024];
   RowTable cnaRows;                /* [5] long longs: step, atoms of type OTHER, FCC, HCP, ICO */
   int* cnaLast;                    /* [nGlobal]: type by gid of the last sample (--cnaDump) */
   long long cnaNonFccNow;          /* the NonFCC column of printThings: the last sample */
   /* box deformation (--erateX/Y/Z, comdSetBox, comdSetStrainRate): the box is box0 (1 + strain), strain = deformEpsBase + erate * deformTime / 1000 */
   double box0[3];                  /* the global extents the simulation was created with */
   double erate[3];                 /* strain rates in 1/ps */
   int deform;                      /* a rate is non-zero: timestep() sets the box at the top of every step from deformStart on */
   int deformStart;
   double deformTime;               /* fs strained at the current rates */
   double deformEpsBase[3];         /* the strain the current rates started from */
   double nextExtent[3];            /* the extents the remap of the coming step will set (the current ones when nothing strains): the list rule looks a step ahead */
   double listExtent[3];            /* *_nl: the global extents at the last list build */
   int boxChanged;                  /* comdSetBox has changed the box at least once: g(r) is normalised with the mean density of its samples */
   double rdfDensitySum;            /* sum over the g(r) samples of N / V */
   int deformReport;                /* the Deform report (reports.c): the V/V0 and Sxx(GPa) columns of printThings, the samples below, the file and the YAML block */
   char deformFile[1024];
   RowTable deformRows;             /* [15] doubles: step, time (fs), strain (3), extents (3), volume, stress xx yy zz yz xz xy (GPa), temperature (K) */
   int stress;                      /* --stress: comdMain samples the per-atom stress summary at every printed step */
   char stressFile[1024], stressDump[1024];
   double stressDumpMin;            /* GPa */
   RowTable stressRows;             /* [8] doubles: step, the seven values of comdStressSummary (eV/A^3) */
   double stressMaxVmNow;           /* the MaxVM(GPa) column of printThings: the last sample, in eV/A^3 */
   int strainHasRef;                /* comdStrainReference: the device holds a reference table */
   double strainL0[3];              /* the global box when the reference was taken */
   int strain, strainRef;           /* --strain: comdMain takes the reference at global step strainRef and samples the summary at every printed step from then on */
   double strainCutoff, strainThreshold, strainDumpMin;      /* r_s (A, default resolved), the shear-strain threshold of the count, that of the dump */
   char strainFile[1024], strainDump[1024];
   RowTable strainRows;             /* [10] doubles: step, the nine values of comdStrainSummary */
   double strainMaxShearNow;        /* the MaxShear column of printThings: the last sample, 0 before the reference */
   int heatflux, hfStart, hfWindow; /* --heatflux: comdMain samples comdHeatFlux at every printed step from global step hfStart on; lags of the autocorrelation (0 = half the samples) */
   char hfFile[1024], hfAcfFile[1024];
   RowTable hfRows;                 /* [13] doubles: step, time (fs), the nine sums of comdHeatFlux (eV A/fs), temperature (K), volume (A^3) */
   double hfJxNow;                  /* the Jx column of printThings: the x component of the flux density of the last sample in eV/A^2/fs, 0 before hfStart */
   /* Berendsen barostat (--baro, comdSetBarostat): every baroEvery steps the step ends unfused, the pressure of comdVirialFdotr gives mu, and the next step's remap
    * sets the box the coupling asked for */
   int baro;                        /* on: timestep() couples */
   double baroTarget[3];            /* GPa, compressive positive */
   double baroTau, baroModulus;     /* fs, GPa */
   int baroEvery, baroAxes, baroIso, baroStart;      /* axes: bit a = axis a is scaled */
   int baroPending;                 /* a coupling has set baroNext: the remap of the coming step applies it */
   double baroNext[3];              /* the extents that remap will set on the barostat's axes */
   int baroReport;                  /* the Barostat report (reports.c): the Pressure(GPa) and V/V0 columns of printThings, the file and the YAML block */
   char baroFile[1024];
   RowTable baroRows;               /* [12] doubles: step, time (fs), p xx yy zz (GPa), mu x y z, L x y z (A), V (A^3) -- the box after the coupling */
   int* facePairs;                  /* comdVirialFdotr: the rows of comdPeriodicFacePairs, built at its first call */
   int nFacePairs;
   /* slab profiles (--profile): comdMain adds comdSlabProfile's integer planes up at every printed step from global step profStart on */
   int profile, profAxis, profBins, profStart;
   char profFile[1024];
   int64_t* profSum;                /* [6][profBins]: the planes of comdSlabProfile summed over the samples */
   int profSamples, profFirstStep, profLastStep;      /* the steps of the first and the last sample */
   double profLSum, profAreaSum;    /* the extent along the axis and the cross-section, summed over the samples */
   /* Mueller-Plathe exchange (--mp, comdSetMullerPlathe): every mpEvery steps the step ends unfused and comdMullerPlatheSwap exchanges momenta behind its closing
    * half kick */
   int mp;                          /* on: timestep() exchanges */
   int mpAxis, mpBins, mpEvery, mpSwaps, mpStart;
   double mpExchanged;              /* eV carried from the cold to the hot slab by all exchanges so far (comdMullerPlatheSwap adds to it) */
   long long mpPairs, mpSkipped, mpExchanges;      /* pairs swapped, pairs asked for and not swapped, exchanges */
   double mpExchangedAtProfStart;   /* mpExchanged after the exchanges of the steps up to global step profStart */
   int mpReport;                    /* the MullerPlathe report (reports.c): the dE(eV) column of printThings; the file and the YAML block come from the profile's writer */
   char mpFile[1024];
   RowTable mpRows;                 /* [6] doubles: step, time (fs), kept pairs, skipped pairs, dE (eV), cumulative E (eV) */
   double* mpTable;                 /* comdMullerPlatheSwap: the candidate table of all ranks and its staging, 2 x [2][nRanks * 64][6] */
   /* structure factor (--sk): at every printed step from global step skStart on comdMain adds the powder average of comdStructureFactor up and samples comdBraggOrder */
   int cells[3];                    /* the unit cells of -x -y -z: the strides of comdBraggOrder */
   int sk, skStride[3], skBins, skStart;      /* sk: the largest index M, 0 = off */
   char skFile[1024];
   double* skSum;                   /* [2][skBins]: per |k| bin the sum of S over the vectors and samples, and the number of vectors summed (h > 0 twice) */
   int skSamples;
   double skBoxSum[3];              /* the extents summed over the samples */
   double skBraggNow, skBraggFirst, skBraggSum;      /* comdBraggOrder of the last sample, of the first, summed over the samples */
   /* Steinhardt order (--steinhardt): comdMain samples comdSteinhardtSummary at every printed step */
   int steinhardt;
   double stSolid, stDumpMax;       /* the q6 threshold of the solid-like count; the dump keeps q6 <= stDumpMax and the invalid atoms */
   char stFile[1024], stDump[1024];
   RowTable stRows;                 /* [11] doubles: step, the ten values of comdSteinhardtSummary */
   double stMeanQ6Now;              /* the MeanQ6 column of printThings: the last sample */
   /* elastic constants (--elastic): comdMain samples comdBornMatrix and the pair stress at every printed step from elStart on */
   int elastic, elStart;
   char elFile[1024];
   RowTable elRows;                 /* [30] doubles: step, T (K), V (A^3), the six pair stresses -W / V and the 21 B / V (eV/A^3) */
   double elC11BornNow;             /* the C11B(GPa) column of printThings: (B11 + B22 + B33) / 3V of the last sample */
} SimFlat;

SimFlat* initSimulation(Command cmd);
SimFlat* initSimulationHost(Command cmd);      /* no device: lattice, momenta, link cells only */
void destroySimulation(SimFlat** ps);
void sumAtoms(SimFlat* s);
void printThings(SimFlat* s, int iStep, double elapsedTime);
Validate* initValidate(SimFlat* s);
void validateResult(const Validate* val, SimFlat* sim);
void printSimulationDataYaml(FILE* file, SimFlat* s);
void setBoundaryCellsHost(SimFlat* sim, HaloExchange* hh);

/* ---- the run-time reports (not in the reference): reports.c, one table row each ---- */
void reportsSample(SimFlat* s, int iStep);                     /* a printed step: every report that is on and has begun samples, each under its timer; collective */
int  reportsNextStart(const SimFlat* s, int iStep, int end);   /* the first step in (iStep, end) at which a report takes its origin or reference; end when none does */
void reportsStart(SimFlat* s, int iStep);                      /* ... and takes it: for such a step between two printed ones */
void reportsColumns(const SimFlat* s, int header);             /* printThings: the reports' part of the header line (header != 0) or of a row */
void reportsWrite(FILE* yaml, SimFlat* s, int iStep);          /* the end of the run: files and YAML blocks; collective */
void reportsFree(SimFlat* s);                                  /* what the reports keep in SimFlat */

/* ---- timestep.h ---- */
double timestep(SimFlat* s, int n, real_t dt);
void computeForce(SimFlat* s);
void kineticEnergyGpu(SimFlat* s);
/* not in the reference: W, K (summed over ranks) and V of the current state, after a complete force evaluation */
void computePressure(SimFlat* s);
/* pressure tensor (K + W) / V in eV/A^3 and its trace / 3, and the conversion to GPa */
#define eVperA3inGPa 160.21766208
double pressureOf(const SimFlat* s);
/* not in the reference: the global histogram of pair distances of the current state (after a complete force evaluation), nBins uniform bins
 * [k dr, (k + 1) dr), dr = rMax / nBins; rMax <= 0 = the force cutoff.  outCounts[k] = unordered pairs in bin k: the ranks' ordered counts
 * (computePairHistogram) summed -- integers below 2^53, exact in doubles -- and halved (every pair is seen once from each side, so the sum is even).
 * The same on every rank.  -1 and nothing launched for nBins < 1, nBins > COMD_RDF_MAX_BINS or rMax > the force cutoff */
#define COMD_RDF_MAX_BINS 4096
int comdPairHistogram(SimFlat* s, int nBins, double rMax, double* outCounts);
/* not in the reference: unwrapped displacements since an origin, accumulated by the drift kernels in 64-bit fixed point per global atom id
 * (include/comd_hip.h comdTrackDisplacementGpu).  Collective: every rank makes each call.
 * comdTrackDisplacement: on != 0 sets (or, when already tracking, resets) the origin to the current state, 0 stops and frees; non-zero, with
 *    nothing tracked on any rank, when a device refuses the memory.
 * comdDisplacements: out[3 gid + {0, 1, 2}] = the global displacement of atom gid in Angstroms, the same on every rank: the ranks' integer records
 *    summed (exact, whatever ranks the atom has been on).  -1 when not tracking, -2 when a component is beyond 2^53 units (2^21 A) on several ranks.
 * comdMsd: out7 = {sum dx, sum dy, sum dz, sum dx^2, sum dy^2, sum dz^2, N} over all atoms.  One rank: the device reduction; several: the sums of
 *    comdDisplacements in gid order on the host (squares of the ranks' parts do not add).  Same return values. */
int comdTrackDisplacement(SimFlat* s, int on);
int comdDisplacements(SimFlat* s, double* out);
int comdMsd(SimFlat* s, double* out7);
/* not in the reference: the centro-symmetry parameter (Angstroms^2, +inf with fewer than 12 neighbours inside the force cutoff) and the coordination
 * number (neighbours closer than rCoord) of every atom of the current state (after a complete force evaluation, as comdPairHistogram), keyed by gid:
 * cspByGid[g], coordByGid[g], nGlobal doubles each.  Each rank fills the entries of its local atoms from computeCentroSymmetry, the others stay 0, and the
 * arrays are summed over the ranks: the same on every rank.  Collective.  rCoord <= 0 = the default, halfway between the first and second FCC shells,
 * (1/sqrt 2 + 1) lat / 2, or the force cutoff where that is smaller.  -1 and nothing launched for rCoord > the force cutoff. */
int comdCentroSymmetry(SimFlat* s, double rCoord, double* cspByGid, double* coordByGid);
double comdDefaultCoordRadius(SimFlat* s);              /* that default */
/* not in the reference: adaptive common neighbour analysis of the current state (valid whenever comdCentroSymmetry is), keyed by gid: typeByGid[g],
 * nGlobal ints, is COMD_CNA_OTHER, _FCC, _HCP or _ICO (OVITO's numbers; 3, BCC, is never returned), and counts[t] the atoms of type t.  Each rank fills
 * the entries of its local atoms from computeCommonNeighbors, the others stay 0, and the array is summed over the ranks: the same on every rank.
 * Collective.  Returns 0. */
enum { COMD_CNA_OTHER = 0, COMD_CNA_FCC = 1, COMD_CNA_HCP = 2, COMD_CNA_BCC = 3, COMD_CNA_ICO = 4 };
int comdCommonNeighbors(SimFlat* s, int* typeByGid, long long counts[5]);
/* not in the reference: the per-atom virial stress of the current state (valid whenever computePressure is), keyed by gid: stressByGid[6 g + c], nGlobal x 6
 * doubles in eV (stress x volume, tension positive), c = xx yy zz yz xz xy; withKinetic != 0 includes -p p^T / m.  Their sum over the atoms is -(W) or
 * -(K + W) of computePressure.  Each rank fills the entries of its local atoms from computeAtomStress, the others stay 0, and the array is summed over the
 * ranks: the same on every rank.  Collective.  -1 and nothing launched on a simulation without device state. */
int comdAtomStress(SimFlat* s, int withKinetic, double* stressByGid);
/* not in the reference: out7 = {mean p, min p, max p, mean sigma, max sigma, the gid that holds it (the lowest of equals), N} of the current state: hydrostatic
 * pressure p and von Mises stress sigma of every atom's tensor over the uniform atomic volume V / N, in eV/A^3 (x eVperA3inGPa = GPa), reduced on the device
 * (computeAtomStress without a copy, computeAtomStressSummary) and then over the ranks.  The same on every rank.  Collective.  -1 as comdAtomStress. */
int comdStressSummary(SimFlat* s, int withKinetic, double* out7);
/* not in the reference: the heat flux of the current state in eV A/fs (flux density x volume; computeHeatFlux, comd_hip.h, has the formulas).  Valid whenever
 * computePressure is AND the per-atom energies are current: after computeForce, comdDeformTo or a timestep() call (the last step of a call asks the force kernels
 * for them), so between the timestep() calls of a run, not inside one.
 * comdHeatFlux: out9 = the sums over all atoms of jk x y z (kinetic convective), jp x y z (potential convective), jv x y z (virial): this rank's sums from the
 *    device reduction, then the sum over the ranks.  J V is the sum of the three parts, the flux density J V / V.  The same on every rank.  Collective.
 * comdAtomHeatFlux: byGid[9 g + c], nGlobal x 9 doubles, the same nine components per atom.  Each rank fills the entries of its local atoms, the others stay
 *    0, and the array is summed over the ranks: the same on every rank.  Collective.
 * Both: -1 and nothing launched on a simulation without device state. */
int comdHeatFlux(SimFlat* s, double out9[9]);
int comdAtomHeatFlux(SimFlat* s, double* byGid);
/* not in the reference: the autocorrelation of a series j[samples][3], acf[3 k + a] = (1 / (samples - k)) sum_t j[t][a] j[t + k][a] for 0 <= k < window, summed in
 * time order in double.  Plain C, no device.  -1 and nothing written unless 1 <= window <= samples. */
int comdHeatFluxAcf(const double* j, int samples, int window, double* acf);
/* not in the reference: the reference snapshot of the per-atom strain.  on != 0: the current positions of all atoms become x0, keyed by gid, in a table of
 * doubles replicated on every rank's device (32 bytes per global atom: each rank stores its local atoms, the tables are summed over the ranks -- every other
 * rank holds 0 for a gid -- and uploaded), and the current global box becomes L0; already on: the reference moves to the current state.  on == 0: it is
 * dropped and the device memory freed.  All ranks or none.  Collective.  Returns 1 when a device refused the memory, -1 without device state, else 0. */
int comdStrainReference(SimFlat* s, int on);
int comdStrainReferenceBox(SimFlat* s, double* L0);      /* L0[3] of the reference; -1 and nothing written without one */
/* not in the reference: the Green-Lagrange strain E = 1/2 (F^T F - I) and the non-affine displacement D^2min of every atom of the current state against the
 * reference (computeAtomStrain, comd_hip.h, says how F is fitted), keyed by gid: strainByGid7[7 g + c], c = 0..5 E xx yy zz yz xz xy, c = 6 D^2 in A^2, and
 * countByGid[g] the neighbours within rCut of the current configuration; NaN in all seven for an invalid atom (fewer than 3 neighbours or a singular V).
 * rCut <= 0: the default, comdDefaultCoordRadius.  Each rank fills the entries of its local atoms, the others stay 0, and the arrays are summed over the
 * ranks (NaN + 0 stays NaN): the same on every rank.  Collective.  -1 and nothing launched without device state, without a reference or for rCut above the
 * force cutoff. */
int comdAtomStrain(SimFlat* s, double rCut, double* strainByGid7, int* countByGid);
/* not in the reference: out9 = {atoms, invalid atoms, mean gamma, max gamma, the gid that holds it (the lowest of equals, -1 without a valid atom), mean
 * tr E / 3, mean D^2, max D^2, atoms with gamma >= threshold} of the current state, gamma the shear invariant of E (computeAtomStrainSummary, comd_hip.h);
 * means and extremes over the valid atoms (0 without any).  Reduced on the device and then over the ranks.  The same on every rank.  Collective.  -1 as
 * comdAtomStrain, or for a threshold that is not > 0. */
int comdStrainSummary(SimFlat* s, double rCut, double threshold, double* out9);
/* not in the reference: Steinhardt's bond-orientational order of every atom of the current state on its 12 nearest neighbours inside the force cutoff
 * (computeSteinhardt, comd_hip.h, has the definitions), keyed by gid: outByGid4[4 g + c], c = 0 q4, 1 q6, 2 w4, 3 w6; NaN in all four for an invalid atom
 * (fewer than 12 neighbours inside the cutoff).  Valid whenever comdCentroSymmetry is.  Each rank fills the entries of its local atoms, the others stay 0, and
 * the array is summed over the ranks (NaN + 0 stays NaN): the same on every rank.  Collective.  -1 and nothing launched without device state. */
int comdSteinhardt(SimFlat* s, double* outByGid4);
/* not in the reference: out10 = {valid atoms, invalid atoms, mean q4, mean q6, min q6, the gid that holds it (the lowest of equals, -1 without a valid atom),
 * max q6, mean w4, mean w6, atoms with q6 >= threshold} of the current state (computeSteinhardtSummary, comd_hip.h); means and extremes over the valid atoms
 * (0 without any).  Reduced on the device and then over the ranks.  The same on every rank.  Collective.  -1 without device state or for a threshold outside
 * (0, 1). */
int comdSteinhardtSummary(SimFlat* s, double threshold, double* out10);
/* not in the reference: born21 = the Born matrix of the current state (computeBornMatrix, comd_hip.h, has the definition), the second derivative of the potential
 * energy with respect to the Lagrangian strain, in eV: the upper triangle of the 6 x 6 matrix in Voigt order xx yy zz yz xz xy, row-major, summed over the
 * ranks.  Valid whenever computePressure is: after a complete force evaluation.  The same on every rank.  Collective.  -1 and nothing launched without device state. */
int comdBornMatrix(SimFlat* s, double* born21);
/* not in the reference: the stress-fluctuation elastic constants (Squire, Holt, Hoover 1969) of nSamples samples of a fixed box, in the units of the input:
 *   C_IJ = <B_IJ> / V - (V / kB T) (<s_I s_J> - <s_I> <s_J>) + (N kB T / V) kappa_IJ,  kappa = diag(2, 2, 2, 1, 1, 1)
 * bornOverV[nSamples][21] the upper triangles of B / V, stress[nSamples][6] the pair stresses -W / V (both eV/A^3), volume in A^3, temperature in K.  With
 * temperature = 0 or fewer than two samples the fluctuation and kinetic parts are 0.  outBorn, outFluct, outKinetic: the three parts, 6 x 6 each, row-major; their
 * sum is C.  Pure arithmetic; -1 for nSamples < 1 or a volume or temperature that is not >= 0. */
int comdElasticConstants(const double* bornOverV, const double* stress, int nSamples, double volume, double temperature, double nAtoms, double* outBorn, double* outFluct, double* outKinetic);
/* not in the reference (its box is nx lat for the whole run): box deformation, LAMMPS's `fix deform ... remap x`.
 * comdSetBox: the global box becomes L[3] Angstroms (the origin stays at 0) and the positions of the local atoms are scaled with it, L_new / L_old per axis, by
 *    comdRemapBoxGpu.  Every copy of the geometry follows: Domain (the expressions of initDecomposition, so neighbouring ranks agree bit for bit on their shared
 *    face), LinkCell (bounds, cell widths, geom; the cell COUNT stays), the periodic shifts of the atom and position exchanges and the mirror path's table of
 *    them, the device's LinkCellGpu.  Momenta, halo cells and the displacement records of comdTrackDisplacement are not touched: a redistribution must follow
 *    before anything reads the cells (timestep() remaps at the top of a step; comdDeformTo does the rest itself).  Collective: every rank makes the call with
 *    the same L.  Returns -1 with NOTHING changed or launched when an L is not positive or a cell would become narrower than the range the grid was built for
 *    (the cutoff, + the skin for the *_nl methods): re-gridding is not implemented.  On a host-only simulation the host geometry alone changes, no atom moves.
 * comdDeformTo: comdSetBox, then a redistribution (with lists: a list build), a force evaluation and an energy read, so that the energy, the virial, the gathered
 *    arrays and the analyses are those of the new state.  -1 as comdSetBox.
 * comdSetStrainRate: engineering strain rates in 1/ps for the coming timestep() calls, from the current box on; all zero = off, and timestep() is then what it was
 *    without the feature, bit for bit.  -1, nothing changed, for a rate that is not finite, with -s (no redistribution there) or on an axis the barostat scales.
 * comdGetBox: out[0..2] the current global extents, out[3..5] those at creation.  comdLocalBounds: out[0..2] this rank's localMin, out[3..5] its localMax. */
int  comdSetBox(SimFlat* s, const double L[3]);
int  comdDeformTo(SimFlat* s, const double L[3]);
int  comdSetStrainRate(SimFlat* s, const double ratesPerPs[3]);
void comdGetBox(SimFlat* s, double out[6]);
void comdLocalBounds(SimFlat* s, double out[6]);
/* not in the reference: pressure coupling.
 * comdPeriodicFacePairs: the work list of computeVirialFdotr (comd_hip.h) from the static neighbour table and the process grid: rows of 5 ints (local cell, halo cell
 *    that holds periodic images, sign x, sign y, sign z; the images sit at home position + sign_a L_a).  Returns the number of rows and writes the first `cap` of them
 *    to out5 (NULL: count only).  Needs no device: it works on a host-only simulation.
 * comdVirialFdotr: comdVirial's twin on the forces of the last force evaluation, {W[6], K[6], V} summed over the ranks; collective; valid after timestep(),
 *    computeForce() or comdDeformTo().  It does not touch the W, K, V that computePressure keeps.
 * comdBerendsenScale: the scale rule, plain C, no device.  mu_a = (1 - (dtCoupling / tau) (target_a - p_a) / modulus)^(1/3) on the axes of axesMask (bit a), 1 on the
 *    others; iso != 0: one mu from the means of p and target over the chosen axes.  p positive when compressive, p_a = (K_aa + W_aa) / V, in the units of target and
 *    modulus; dtCoupling and tau in the same unit of time.  -1 and mu untouched for a non-finite argument, tau <= 0, modulus <= 0, dtCoupling > tau, dtCoupling < 0, an
 *    empty or out-of-range mask or a mu that would not be positive.
 * comdSetBarostat: the barostat for the coming timestep() calls: every `every` steps (those after which stepCount - baroStart is a positive multiple of every) the
 *    step ends unfused, comdVirialFdotr gives p, comdBerendsenScale with dtCoupling = every * dt gives mu, and the remap at the top of the next step sets L_a mu_a on
 *    the chosen axes through comdSetBox.  on == 0: off, timestep() is what it was.  -1 and nothing changed with -s, without device state, for an axis that also has a
 *    non-zero strain rate, every < 1, an empty mask, or what comdBerendsenScale refuses (dtCoupling is checked at timestep(), which knows dt).
 * comdGetBarostat: returns on/off; out8 = {target x y z (GPa), tau (fs), modulus (GPa), every, axesMask, iso}. */
int  comdPeriodicFacePairs(SimFlat* s, int* out5, int cap);
void comdVirialFdotr(SimFlat* s, double out[13]);
int  comdBerendsenScale(const double p[3], const double target[3], double dtCoupling, double tau, double modulus, int axesMask, int iso, double mu[3]);
int  comdSetBarostat(SimFlat* s, int on, const double targetGPa[3], double tauFs, double modulusGPa, int every, int axesMask, int iso);
int  comdGetBarostat(SimFlat* s, double out8[8]);
int  comdBarostatRefusal(const SimFlat* s, const double targetGPa[3], double tauFs, double modulusGPa, int every, int axesMask);      /* why comdSetBarostat would refuse, 0 = it would not */
/* not in the reference: slab profiles and the Mueller-Plathe exchange (hip/profile_kernels.h, hip/mp_kernels.h).  Collective: every rank makes each call.
 * comdSlabProfile: the six integer planes of computeSlabProfile (comd_hip.h) on the current global extent of `axis`, summed over the ranks: out6xN[c * nBins + b],
 *    c = count, sum p_x, p_y, p_z, sum KE, sum e, the sums of reals in units of 2^-32.  The rank sum is exact: every 64-bit word travels as two 32-bit halves, each a
 *    double, through addDoubleParallel, and is put together again in integers.  The same on every rank.  -1, nothing launched, without device state, for an axis
 *    outside 0..2 or nBins outside 1..COMD_PROFILE_MAX_BINS.
 * comdMullerPlatheRefusal: why an exchange setting is refused: 0 fine, 1 the axis, 2 the bins (outside 1..1024, odd or fewer than 4), 3 every < 1, 4 swaps outside 1..64.
 * comdMullerPlatheCandidates: the candidate table of all ranks: table[(l * nRanks * k + r) * 6 ...], l = 0 the cold list (slab 0, hottest first), 1 the hot list (slab
 *    nBins / 2, coldest first), rows r = rank * k + j.  A row is {KE, gid + 1, p_x, p_y, p_z, slot on its rank}; a row of zeros is empty (a rank whose share of the slab
 *    holds fewer than k atoms).  Each rank fills its rows of a zeroed table and addDoubleParallel delivers the sum: the same on every rank.  -1 as comdMullerPlatheSwap.
 * comdMullerPlatheTop: plain C.  The list order itself: top[0 .. n - 1] are the indices of the first n <= k non-empty rows of `rows` in list order (hot != 0: KE ascending,
 *    else KE descending; the lower gid first among equal KE); returns n.  What comdMullerPlatheMatch takes its two lists with.
 * comdMullerPlatheMatch: plain C, no device, no transport.  cold and hot are such rows, nCold and nHot of them.  The global top k of each list in list order -- by
 *    (KE, gid): cold KE descending, hot KE ascending, the lower gid first among equal KE -- are paired rank for rank, the j-th hottest of the cold slab with the j-th
 *    coldest of the hot slab, and a pair is kept while KE of the cold-slab atom > KE of the hot-slab atom: from the first pair that fails on all are dropped (LAMMPS's
 *    rule).  Returns the number of kept pairs; pairs[2 j], pairs[2 j + 1] are the ROW indices of pair j in cold and hot; *deltaE = sum (KE_cold-slab - KE_hot-slab).
 * comdMullerPlatheSwap: one exchange on the current state: candidates, match, and MP_apply on the atoms this rank owns -- the two momentum vectors of a pair change
 *    places bit for bit (one mass: the project has one species).  Positions, forces and everything else stay.  pairsGid[2 j], [2 j + 1]: the gids of pair j (cold-slab
 *    atom, hot-slab atom), room for k pairs.  *skipped = k - kept: pairs asked for and not made, for lack of atoms or by the KE rule.  Adds to the tally
 *    (mpExchanged, mpPairs, mpSkipped, mpExchanges).  Returns kept, or -1 without device state or for what comdMullerPlatheRefusal refuses.
 * comdSetMullerPlathe: the exchange for the coming timestep() calls: at the end of every step whose global count s + 1 > start and (s + 1 - start) % every == 0 the
 *    step ends unfused (as a barostat coupling step does) and comdMullerPlatheSwap runs behind its closing half kick.  on == 0: off, timestep() is what it was; the
 *    tally stays.  -1 and nothing changed without device state, for start < 0 or what comdMullerPlatheRefusal refuses.
 * comdGetMullerPlathe: returns on/off; out8 = {axis, bins, every, swaps, start, exchanged (eV), pairs, skipped}.
 * comdFourierKappa: plain C.  T[nBins] the time-averaged slab temperatures (K; NaN: an empty slab), width the slab width (A), area the cross-section (A^2), energy
 *    the eV exchanged in `time` fs.  The two halves are folded, bin b with bin nBins - b for 0 < b < nBins / 2, and a least-squares line goes through the folded
 *    temperatures of those interior bins against b * width; *gradient = |slope| in K/A; q = energy / (2 area time); *kappa = q / gradient in W/(m K)
 *    (1 eV/(fs A K) = 1.602176634e6 W/(m K)).  Returns 0; 1 when there is a gradient and no kappa (gradient 0, or area, time not positive); -1, nothing written,
 *    with fewer than two interior bins that have a temperature in both halves, or an odd nBins. */
#define COMD_PROFILE_MAX_BINS 1024
#define COMD_MP_MAX_SWAPS 64
int  comdSlabProfile(SimFlat* s, int axis, int nBins, int64_t* out6xN);
int  comdMullerPlatheRefusal(int axis, int nBins, int every, int swaps);
int  comdMullerPlatheCandidates(SimFlat* s, int axis, int nBins, int k, double* table);
int  comdMullerPlatheTop(const double* rows, int nRows, int k, int hot, int* top);
int  comdMullerPlatheMatch(const double* cold, int nCold, const double* hot, int nHot, int k, int* pairs, double* deltaE);
int  comdMullerPlatheSwap(SimFlat* s, int axis, int nBins, int k, int* pairsGid, double* deltaE, int* skipped);
int  comdSetMullerPlathe(SimFlat* s, int on, int axis, int nBins, int every, int swaps, int start);
int  comdGetMullerPlathe(SimFlat* s, double out8[8]);
int  comdFourierKappa(const double* T, int nBins, double width, double area, double energy, double time, double* gradient, double* kappa);
/* not in the reference: the static structure factor (hip/sk_kernels.h).  comdStructureFactor and comdBraggOrder are collective: every rank makes each call.
 * comdStructureFactorRefusal: why a grid is refused: 0 fine, 1 M outside 1..COMD_SK_MAX_M, 2 a stride < 1, 3 a stride * M above COMD_SK_MAX_HM.
 * comdStructureFactor: the density amplitudes rho(h, k, l) = sum_j exp(-i K . r_j) over the atoms of all ranks, K = 2 pi (stride[0] h / Lx, stride[1] k / Ly,
 *    stride[2] l / Lz) on the current global extents, h in [0, M], k, l in [-M, M]: outKx2[((h W + k + M) W + l + M) 2 + {0, 1}], W = 2M + 1, real and imaginary
 *    part.  computeStructureFactor (comd_hip.h) for this rank's atoms, summed over the ranks with addDoubleParallelLong: the same on every rank.  rho(0, 0, 0) is N
 *    exactly.  One configuration gives the same bits at every call; methods, cell numberings and rank counts order the atoms differently and differ in the
 *    rounding.  Returns what comdStructureFactorRefusal does, nothing launched; -1 without device state.
 * comdStructureFactorRadial: plain C, no device: the powder average of such amplitudes on a box of extents box[3].  S = |rho|^2 / N with N = Re rho(0, 0, 0).
 *    nBins uniform |k| bins up to kMax = min_a 2 pi stride[a] M / box[a], the largest sphere inside the grid: a vector with 0 < |k| <= kMax is in bin
 *    min(floor(|k| / (kMax / nBins)), nBins - 1), K_a = (2 pi (stride[a] index)) / box[a], |k| = sqrt((Kx^2 + Ky^2) + Kz^2).  A vector with h > 0 counts twice (it
 *    stands for -K too), one with h = 0 once (the plane holds both); K = 0 is left out.  kCentre[b] = (b + 0.5) kMax / nBins, count[b] the weights, sMean[b] the
 *    weighted mean of S, NaN where count is 0.  Returns what comdStructureFactorRefusal does, 4 for nBins outside 1..COMD_SK_MAX_BINS, 5 for a box extent or an N
 *    that is not positive.
 * comdBraggOrder: the mean over the four reflections (1, +-1, +-1) of S / N at the strides (nx, ny, nz) of -x -y -z, the {111} family of the conventional cubic
 *    cell: 1 on the perfect lattice, the Debye-Waller factor of a warm crystal, ~1/N in the melt.  One comdStructureFactor call with M = 1.  -1 without device state. */
#define COMD_SK_MAX_M 64
#define COMD_SK_MAX_HM 65536
#define COMD_SK_MAX_BINS 4096
int  comdStructureFactorRefusal(int M, const int stride[3]);
int  comdStructureFactor(SimFlat* s, int M, const int stride[3], double* outKx2);
int  comdStructureFactorRadial(const double* rhoKx2, int M, const int stride[3], const double box[3], int nBins, double* kCentre, double* sMean, double* count);
int  comdBraggOrder(SimFlat* s, double* out);
void deformListBudget(SimFlat* s);      /* *_nl: the skin left to the displacement test by the compression since the build; after a box change and after a list build */
void redistributeAtoms(SimFlat* sim);
void ensureInteriorForceLaunched(SimFlat* sim);

/* ---- performanceTimers.h ---- */
enum TimerHandle { totalTimer, loopTimer, timestepTimer, positionTimer, velocityTimer, redistributeTimer, atomHaloTimer,
                   computeForceTimer, eamHaloTimer, commHaloTimer, commReduceTimer, neighborListBuildTimer, pressureTimer, rdfTimer, msdTimer, cspTimer, cnaTimer, deformTimer, stressTimer, strainTimer, heatfluxTimer, baroTimer, profileTimer, mpTimer, skTimer, steinhardtTimer, elasticTimer, numberOfTimers };
void profileStart(enum TimerHandle handle);
void profileStop(enum TimerHandle handle);
double getElapsedTime(enum TimerHandle handle);
void resetTimers(void);
/* device-true timing: every start/stop of a phase of timestep() also records a HIP event on `stream`; the report then shows device seconds for those
 * phases (same table, same YAML keys) and adds atomUpdatesPerSec / forceKernelGBs.  forceBytesPerAtom: algorithmic bytes of one force evaluation. */
void timersUseDevice(int on, comdStream_t stream, double forceBytesPerAtom);
void printPerformanceResults(int nGlobalAtoms, int printRate);
void printPerformanceResultsYaml(FILE* file);
#define startTimer(h) profileStart(h)
#define stopTimer(h)  profileStop(h)

/* ---- yamlOutput.h ---- */
extern FILE* yamlFile;
void yamlBegin(void);
void yamlEnd(void);
void yamlAppInfo(FILE* file);
void printSeparator(FILE* file);

/* ---- embedding API (Python/ctypes, tests, bench): a thin layer over the functions above ---- */
SimFlat* comdCreate(int argc, char** argv);              /* parse the reference CLI, initSimulation */
SimFlat* comdCreateHostOnly(int argc, char** argv);      /* parse + initSimulationHost (CPU tests) */
const HostAtoms* comdHostAtoms(SimFlat* s);              /* the host mirror, without touching the device */
int      comdSimBoxFromTuple(SimFlat* s, int ix, int iy, int iz);
int      comdSimBoxFromCoord(SimFlat* s, const double r[3]);
int      comdFaceCells(SimFlat* s, int kind, int face, int* list);
void     comdNeighborRanks(SimFlat* s, int nbr[6], int coord[3]);
void     comdHaloExchangeHost(SimFlat* s, int (*load)(void*, void*, int, char*), void (*unload)(void*, void*, int, int, char*));
void     comdFaceShift(SimFlat* s, int face, double out[3]);
int      comdPutAtomInBox(SimFlat* s, int gid, int type, const double r[3], const double p[3]);
int      comdEamTable(SimFlat* s, int which, double* x0, double* invDx, double* values);   /* 0 phi, 1 rho, 2 F; n + 3 padded samples */
int      comdLjTable(SimFlat* s, double* x0, double* invDx, double* values);              /* -I: n + 4 padded samples; 0 without -I */
int      comdNeighborListBuilds(SimFlat* s);              /* Verlet-list builds so far (*_nl methods) */
/* not in the reference: the Langevin thermostat from the next timestep() call on (on = 0: NVE again).  -1 and nothing changed if tempK < 0 or
 * tauFs <= 0 */
int      comdSetLangevin(SimFlat* s, double tempK, double tauFs, uint64_t seed, int on);
int      comdGetLangevin(SimFlat* s, double out[2], uint64_t* seed);    /* on/off; out = {tempK, tauFs} */
uint64_t comdStepCount(SimFlat* s);                       /* steps taken since creation */
void     comdVirial(SimFlat* s, double out[13]);          /* computePressure, then {W[6], K[6], V}: global pair virial and kinetic tensor (eV), volume (A^3) */
double   comdCutoff(SimFlat* s);                          /* the force cutoff in Angstroms: the largest rMax of comdPairHistogram, and its default */
double   comdLatticeConstant(SimFlat* s);                 /* the lattice constant the crystal was made with, in Angstroms: lat^2 / 4 is the default defect threshold */
double   comdVolume(SimFlat* s);                          /* volume of the global domain in A^3 */
double   comdAtomMass(SimFlat* s);                        /* the mass of the (one) species in the project's units, eV fs^2/A^2: v = p / mass */
void     comdGridInfo(SimFlat* s, int out[6]);            /* gridSize[3], nLocalBoxes, nTotalBoxes, maxAtoms */
int      comdMain(int argc, char** argv);                /* the reference's main(): CoMD.c:86-187 */
void     comdDestroy(SimFlat* s);
SimGpu*  comdSimGpu(SimFlat* s);                          /* the device half, for the comd_hip.h calls that take a SimGpu* (force timing) */
void     comdGetEnergy(SimFlat* s, double out[3]);       /* ePotential, eKinetic, nGlobal */
int      comdNumGlobal(SimFlat* s);
int      comdNumLocalSlots(SimFlat* s);                  /* nTotalBoxes * maxAtoms */
/* copy device state to the host mirror and return pointers into it (valid until the next call) */
const HostAtoms* comdFetchAtoms(SimFlat* s);
/* per-atom arrays of this rank's local atoms keyed by gid: which 0 r,1 p,2 f (3 doubles) / 3 e, 4 rhobar, 5 dfEmbed (1 double).
 * `out` must be zero-initialised by the caller when ranks are to be summed. */
void     comdGatherByGid(SimFlat* s, int which, double* out);
/* overwrite r or p of local atoms from a by-gid array (which 0 / 1), then upload */
void     comdScatterByGid(SimFlat* s, int which, const double* in);

#endif
