"""ctypes binding of the MI355X CoMD hot path (libcomd_host.so + libcomd_hip.so).

This is plumbing for tests and bench.py: every call goes through the C ABI declared in
include/comd_hip.h and comd-cuda-async_amd/csrc/host/comd_host.h.  There is no Python or CPU
fallback: if the HIP library is missing, loading fails with an ImportError that says how to build it.

The directory name contains '-', so import it with `__graft_entry__.load_package()`.
"""
import ctypes
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
REPO_ROOT = os.path.dirname(_HERE)
POT_DIR = os.path.join(REPO_ROOT, "pots")

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int_p = ctypes.POINTER(ctypes.c_int)

# One build per precision (make PRECISION=single -> lib*_sp.so, real_t = float: the reference's DOUBLE_PRECISION = OFF, mytype.h:8-21).
# A process binds ONE of them: COMD_PRECISION=single selects the float build before the first library is loaded.
PRECISION = os.environ.get("COMD_PRECISION", "double")
if PRECISION not in ("double", "single"):
    raise ImportError(f"COMD_PRECISION={PRECISION!r}: expected 'double' or 'single'")
_SFX = "_sp" if PRECISION == "single" else ""
c_real = ctypes.c_float if PRECISION == "single" else ctypes.c_double
c_real_p = ctypes.POINTER(c_real)

# structure types of Simulation.common_neighbor_analysis(): OVITO's numbers (3, BCC, is never returned)
CNA_OTHER, CNA_FCC, CNA_HCP, CNA_ICO = 0, 1, 2, 4
# GPa per eV/A^3: the unit of Simulation.pressure(), atomic_pressure(), von_mises() and stress_summary() into the one comd-hip prints
GPA_PER_EV_A3 = 160.21766208


class HostAtoms(ctypes.Structure):
    """include/comd_hip.h HostAtoms"""
    _fields_ = [("nAtoms", c_int_p), ("gid", c_int_p), ("iSpecies", c_int_p)] + \
               [(n, c_real_p) for n in ("rx", "ry", "rz", "px", "py", "pz", "fx", "fy", "fz", "e")]


SENDRECV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                               ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p)
SENDRECV2_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                ctypes.POINTER(ctypes.c_int))
ALLREDUCE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int)
BCAST_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int)
BARRIER_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p)
SENDRECV2SIZED_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p)


LOAD_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p)
UNLOAD_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p)


class CommTransport(ctypes.Structure):
    """include/comd_hip.h CommTransport"""
    _fields_ = [("ctx", ctypes.c_void_p), ("sendrecv", SENDRECV_FN), ("sendrecv2", SENDRECV2_FN), ("allreduce", ALLREDUCE_FN),
                ("bcast", BCAST_FN), ("barrier", BARRIER_FN), ("sendrecv2sized", SENDRECV2SIZED_FN)]


_libs = {}


def _load(name):
    if name in _libs:
        return _libs[name]
    path = os.path.join(_CSRC, name)
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `make -C {_CSRC}{' PRECISION=single' if _SFX else ''}` (hipcc --offload-arch=gfx950). "
                          "There is no CPU fallback for the product path.")
    _libs[name] = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    return _libs[name]


def lib_hip():
    """libcomd_hip.so: HIP kernels + C-ABI launch wrappers."""
    lib = _load(f"libcomd_hip{_SFX}.so")
    if not getattr(lib, "_typed", False):
        lib.SetupGpu.argtypes = [ctypes.c_int] * 3
        lib.SetupGpu.restype = ctypes.c_int
        lib.comdDeviceCount.restype = ctypes.c_int
        lib.comdCommGetUniqueId.argtypes = [ctypes.c_char_p]
        lib.comdCommInitRank.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(CommTransport)]
        lib.comdForceTimingEnable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.comdForceTimingReset.argtypes = [ctypes.c_void_p]
        lib.comdForceTimingTotalMs.argtypes = [ctypes.c_void_p, c_int_p]
        lib.comdForceTimingTotalMs.restype = ctypes.c_double
        lib.comdForceTimingAuxMs.argtypes = [ctypes.c_void_p, c_int_p]
        lib.comdForceTimingAuxMs.restype = ctypes.c_double
        lib.comdDeviceMemInfo.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long)]
        lib.comdCommInitFromEnv.argtypes = [ctypes.POINTER(CommTransport), c_int_p, c_int_p, c_int_p]
        lib.comdCommInitFromEnv.restype = ctypes.c_int
        lib.comdCommInfo.argtypes = [c_int_p, c_int_p, c_int_p]
        lib.comdCommInfo.restype = ctypes.c_int
        lib.comdEventCreate.restype = ctypes.c_void_p
        lib.comdEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.comdEventElapsedMs.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.comdEventElapsedMs.restype = ctypes.c_float
        lib.comdEventDestroy.argtypes = [ctypes.c_void_p]
        lib.comdStreamSynchronize.argtypes = [ctypes.c_void_p]
        lib.comdMemcpyDtoH.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
        lib.comdMemcpyHtoD.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
        lib._typed = True
    return lib


def lib_host():
    """libcomd_host.so: the C host (CLI, decomposition, link cells, potentials, halo exchange, time step)."""
    lib_hip()
    lib = _load(f"libcomd_host{_SFX}.so")
    if not getattr(lib, "_typed", False):
        vp = ctypes.c_void_p
        lib.comdCreate.restype = vp
        lib.comdCreate.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)]
        lib.comdCreateHostOnly.restype = vp
        lib.comdCreateHostOnly.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)]
        lib.comdMain.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)]
        lib.comdDestroy.argtypes = [vp]
        lib.comdSimGpu.argtypes = [vp]
        lib.comdSimGpu.restype = vp
        lib.comdGetEnergy.argtypes = [vp, c_double_p]
        lib.comdNumGlobal.argtypes = [vp]
        lib.comdNumLocalSlots.argtypes = [vp]
        lib.comdFetchAtoms.argtypes = [vp]
        lib.comdFetchAtoms.restype = ctypes.POINTER(HostAtoms)
        lib.comdHostAtoms.argtypes = [vp]
        lib.comdHostAtoms.restype = ctypes.POINTER(HostAtoms)
        lib.comdGridInfo.argtypes = [vp, c_int_p]
        lib.comdEamTable.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_void_p]
        lib.comdLjTable.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_void_p]
        lib.comdLjTable.restype = ctypes.c_int
        lib.comdEamTable.restype = ctypes.c_int
        lib.comdVirial.argtypes = [vp, c_double_p]
        lib.comdPairHistogram.argtypes = [vp, ctypes.c_int, ctypes.c_double, c_double_p]
        lib.comdPairHistogram.restype = ctypes.c_int
        lib.comdTrackDisplacement.argtypes = [vp, ctypes.c_int]
        lib.comdTrackDisplacement.restype = ctypes.c_int
        lib.comdDisplacements.argtypes = [vp, c_double_p]
        lib.comdDisplacements.restype = ctypes.c_int
        lib.comdMsd.argtypes = [vp, c_double_p]
        lib.comdMsd.restype = ctypes.c_int
        lib.comdCentroSymmetry.argtypes = [vp, ctypes.c_double, c_double_p, c_double_p]
        lib.comdCentroSymmetry.restype = ctypes.c_int
        lib.comdCommonNeighbors.argtypes = [vp, c_int_p, ctypes.POINTER(ctypes.c_longlong)]
        lib.comdCommonNeighbors.restype = ctypes.c_int
        lib.comdAtomStress.argtypes = [vp, ctypes.c_int, c_double_p]
        lib.comdAtomStress.restype = ctypes.c_int
        lib.comdStressSummary.argtypes = [vp, ctypes.c_int, c_double_p]
        lib.comdStressSummary.restype = ctypes.c_int
        lib.comdHeatFlux.argtypes = [vp, c_double_p]
        lib.comdHeatFlux.restype = ctypes.c_int
        lib.comdAtomHeatFlux.argtypes = [vp, c_double_p]
        lib.comdAtomHeatFlux.restype = ctypes.c_int
        lib.comdHeatFluxAcf.argtypes = [c_double_p, ctypes.c_int, ctypes.c_int, c_double_p]
        lib.comdHeatFluxAcf.restype = ctypes.c_int
        lib.comdAtomMass.argtypes = [vp]
        lib.comdAtomMass.restype = ctypes.c_double
        lib.comdStrainReference.argtypes = [vp, ctypes.c_int]
        lib.comdStrainReference.restype = ctypes.c_int
        lib.comdAtomStrain.argtypes = [vp, ctypes.c_double, c_double_p, c_int_p]
        lib.comdAtomStrain.restype = ctypes.c_int
        lib.comdStrainSummary.argtypes = [vp, ctypes.c_double, ctypes.c_double, c_double_p]
        lib.comdStrainSummary.restype = ctypes.c_int
        lib.comdSteinhardt.argtypes = [vp, c_double_p]
        lib.comdSteinhardt.restype = ctypes.c_int
        lib.comdSteinhardtSummary.argtypes = [vp, ctypes.c_double, c_double_p]
        lib.comdSteinhardtSummary.restype = ctypes.c_int
        lib.comdBornMatrix.argtypes = [vp, c_double_p]
        lib.comdBornMatrix.restype = ctypes.c_int
        lib.comdElasticConstants.argtypes = [c_double_p, c_double_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_double_p, c_double_p, c_double_p]
        lib.comdElasticConstants.restype = ctypes.c_int
        lib.comdStrainReferenceBox.argtypes = [vp, c_double_p]
        lib.comdStrainReferenceBox.restype = ctypes.c_int
        lib.comdDefaultCoordRadius.argtypes = [vp]
        lib.comdDefaultCoordRadius.restype = ctypes.c_double
        lib.comdLatticeConstant.argtypes = [vp]
        lib.comdLatticeConstant.restype = ctypes.c_double
        lib.comdCutoff.argtypes = [vp]
        lib.comdCutoff.restype = ctypes.c_double
        lib.comdVolume.argtypes = [vp]
        lib.comdVolume.restype = ctypes.c_double
        lib.comdSetBox.argtypes = [vp, c_double_p]
        lib.comdSetBox.restype = ctypes.c_int
        lib.comdDeformTo.argtypes = [vp, c_double_p]
        lib.comdDeformTo.restype = ctypes.c_int
        lib.comdSetStrainRate.argtypes = [vp, c_double_p]
        lib.comdSetStrainRate.restype = ctypes.c_int
        lib.comdGetBox.argtypes = [vp, c_double_p]
        lib.comdVirialFdotr.argtypes = [vp, c_double_p]
        lib.comdPeriodicFacePairs.argtypes = [vp, c_int_p, ctypes.c_int]
        lib.comdPeriodicFacePairs.restype = ctypes.c_int
        lib.comdBerendsenScale.argtypes = [c_double_p, c_double_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, c_double_p]
        lib.comdBerendsenScale.restype = ctypes.c_int
        lib.comdSetBarostat.argtypes = [vp, ctypes.c_int, c_double_p, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        lib.comdSetBarostat.restype = ctypes.c_int
        lib.comdGetBarostat.argtypes = [vp, c_double_p]
        lib.comdGetBarostat.restype = ctypes.c_int
        c_int64_p = ctypes.POINTER(ctypes.c_int64)
        lib.comdSlabProfile.argtypes = [vp, ctypes.c_int, ctypes.c_int, c_int64_p]
        lib.comdSlabProfile.restype = ctypes.c_int
        lib.comdMullerPlatheRefusal.argtypes = [ctypes.c_int] * 4
        lib.comdMullerPlatheRefusal.restype = ctypes.c_int
        lib.comdMullerPlatheCandidates.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p]
        lib.comdMullerPlatheCandidates.restype = ctypes.c_int
        lib.comdMullerPlatheTop.argtypes = [c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_int_p]
        lib.comdMullerPlatheTop.restype = ctypes.c_int
        lib.comdMullerPlatheMatch.argtypes = [c_double_p, ctypes.c_int, c_double_p, ctypes.c_int, ctypes.c_int, c_int_p, c_double_p]
        lib.comdMullerPlatheMatch.restype = ctypes.c_int
        lib.comdMullerPlatheSwap.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_int_p, c_double_p, c_int_p]
        lib.comdMullerPlatheSwap.restype = ctypes.c_int
        lib.comdSetMullerPlathe.argtypes = [vp] + [ctypes.c_int] * 6
        lib.comdSetMullerPlathe.restype = ctypes.c_int
        lib.comdGetMullerPlathe.argtypes = [vp, c_double_p]
        lib.comdGetMullerPlathe.restype = ctypes.c_int
        lib.comdFourierKappa.argtypes = [c_double_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_double_p, c_double_p]
        lib.comdFourierKappa.restype = ctypes.c_int
        lib.comdStructureFactorRefusal.argtypes = [ctypes.c_int, c_int_p]
        lib.comdStructureFactorRefusal.restype = ctypes.c_int
        lib.comdStructureFactor.argtypes = [vp, ctypes.c_int, c_int_p, c_double_p]
        lib.comdStructureFactor.restype = ctypes.c_int
        lib.comdStructureFactorRadial.argtypes = [c_double_p, ctypes.c_int, c_int_p, c_double_p, ctypes.c_int, c_double_p, c_double_p, c_double_p]
        lib.comdStructureFactorRadial.restype = ctypes.c_int
        lib.comdBraggOrder.argtypes = [vp, c_double_p]
        lib.comdBraggOrder.restype = ctypes.c_int
        lib.comdLocalBounds.argtypes = [vp, c_double_p]
        lib.comdSetLangevin.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_uint64, ctypes.c_int]
        lib.comdSetLangevin.restype = ctypes.c_int
        lib.comdGetLangevin.argtypes = [vp, c_double_p, ctypes.POINTER(ctypes.c_uint64)]
        lib.comdGetLangevin.restype = ctypes.c_int
        lib.comdStepCount.argtypes = [vp]
        lib.comdStepCount.restype = ctypes.c_uint64
        lib.comdNeighborListBuilds.argtypes = [vp]
        lib.comdNeighborListBuilds.restype = ctypes.c_int
        lib.comdSimBoxFromTuple.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        lib.comdSimBoxFromCoord.argtypes = [vp, c_double_p]
        lib.comdFaceCells.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.comdNeighborRanks.argtypes = [vp, c_int_p, c_int_p]
        lib.comdHaloExchangeHost.argtypes = [vp, LOAD_FN, UNLOAD_FN]
        lib.comdFaceShift.argtypes = [vp, ctypes.c_int, c_double_p]
        lib.comdPutAtomInBox.argtypes = [vp, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p]
        lib.comdGatherByGid.argtypes = [vp, ctypes.c_int, c_double_p]
        lib.comdScatterByGid.argtypes = [vp, ctypes.c_int, c_double_p]
        lib.timestep.argtypes = [vp, ctypes.c_int, c_real]
        lib.timestep.restype = ctypes.c_double
        for fn in ("redistributeAtoms", "computeForce", "kineticEnergyGpu", "sumAtoms"):
            getattr(lib, fn).argtypes = [vp]
        lib.initParallel.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(CommTransport)]
        lib.getMyRank.restype = ctypes.c_int
        lib.getNRanks.restype = ctypes.c_int
        lib._typed = True
    return lib


def _argv(args):
    argv = [b"comd"] + [str(a).encode() for a in args]
    arr = (ctypes.c_char_p * (len(argv) + 1))(*argv, None)
    return len(argv), arr


def setup_gpu(device=0, rank=0, verbose=False):
    """SetupGpu (gpu_utility.c:32-71).  Raises if no HIP device is visible."""
    hip = lib_hip()
    if hip.comdDeviceCount() < 1:
        raise RuntimeError("no HIP device visible: the product path has no CPU fallback")
    return hip.SetupGpu(device, rank, 1 if verbose else 0)


def init_parallel(rank=0, n_ranks=1, transport=None):
    lib_host().initParallel(rank, n_ranks, ctypes.byref(transport) if transport is not None else None)


def rccl_transport(rank, n_ranks, unique_id):
    """Join the RCCL communicator (after setup_gpu) and return the transport to hand to init_parallel."""
    t = CommTransport()
    rc = lib_hip().comdCommInitRank(unique_id, rank, n_ranks, ctypes.byref(t))
    if rc != 0:
        raise RuntimeError("comdCommInitRank failed")
    return t


def rccl_transport_from_env():
    """Join the RCCL communicator the way comd-hip does (comdCommInitFromEnv: RANK / WORLD_SIZE / LOCAL_RANK, rendezvous through a file keyed by
    the launcher's pid).  No torch, no second HIP runtime in the process.  Returns the transport, or None when the communicator cannot be formed."""
    t = CommTransport()
    r, n, l = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    if lib_hip().comdCommInitFromEnv(ctypes.byref(t), ctypes.byref(r), ctypes.byref(n), ctypes.byref(l)) != 0:
        return None
    return t


def device_mem_info():
    f, t = ctypes.c_long(0), ctypes.c_long(0)
    lib_hip().comdDeviceMemInfo(ctypes.byref(f), ctypes.byref(t))
    return f.value, t.value


def rccl_comm_info():
    """(ranks, my rank, device) as the RCCL communicator itself reports them (ncclCommCount / UserRank / CuDevice)."""
    n, r, d = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    if lib_hip().comdCommInfo(ctypes.byref(n), ctypes.byref(r), ctypes.byref(d)) != 0:
        raise RuntimeError("no RCCL communicator")
    return n.value, r.value, d.value


def mapped_libraries(pattern):
    """Paths of the shared objects mapped into this process whose name contains `pattern` (from /proc/self/maps)."""
    out = []
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split()[-1]
            if pattern in os.path.basename(path) and path not in out:
                out.append(path)
    return out


def rccl_unique_id():
    buf = ctypes.create_string_buffer(128)
    if lib_hip().comdCommGetUniqueId(buf) != 0:
        raise RuntimeError("comdCommGetUniqueId failed")
    return buf.raw


def _whole_pairs(np, halved):
    """int64 pair counts from comdPairHistogram's halved ordered counts.  A pair whose two sides (it is seen once from either atom, across a
    periodic face against a shifted image) round to different sides of a bin edge leaves a half in each of two neighbouring bins.  The
    cumulative sums are floored, which moves each such pair whole into the upper of its two bins: the total is exact and no pair is lost."""
    below = np.floor(np.concatenate([[0.0], np.cumsum(halved)]))      # multiples of 1/2 below 2^53: the sums are exact
    return np.diff(below).astype(np.int64)


class Simulation:
    """One rank's SimFlat (CoMDTypes.h:75-135) driven through the C ABI.

    args are the reference's CoMD command-line flags, e.g. ["-x", 20, "-y", 20, "-z", 20, "-m", "thread_atom"].
    """

    def __init__(self, args, host_only=False):
        import numpy as np
        self._np = np
        self.lib = lib_host()
        args = list(args)
        if "-d" not in args and "--potDir" not in args:
            args += ["-d", POT_DIR]
        if "--quiet" not in args:
            args += ["--quiet"]
        argc, argv = _argv(args)
        self.host_only = host_only
        self.ptr = (self.lib.comdCreateHostOnly if host_only else self.lib.comdCreate)(argc, argv)
        if not self.ptr:
            raise RuntimeError("simulation creation failed")
        info = (ctypes.c_int * 6)()
        self.lib.comdGridInfo(self.ptr, info)
        self.grid = tuple(info[0:3])
        self.n_local_boxes, self.n_total_boxes, self.max_atoms = info[3], info[4], info[5]

    # --- time stepping (timestep.c) ---
    def step(self, n, dt=1.0):
        return self.lib.timestep(self.ptr, n, dt)

    def redistribute(self):
        self.lib.redistributeAtoms(self.ptr)

    def compute_force(self):
        self.lib.computeForce(self.ptr)

    def eam_table(self, which):
        """(x0, invDx, padded samples) of the EAM table 0 phi / 1 rho / 2 F as the host hands it to AllocateGpu."""
        import numpy as np
        x0, inv = ctypes.c_double(), ctypes.c_double()
        n = self.lib.comdEamTable(self.ptr, which, ctypes.byref(x0), ctypes.byref(inv), None)
        v = np.empty(n + 3)
        self.lib.comdEamTable(self.ptr, which, ctypes.byref(x0), ctypes.byref(inv), v.ctypes.data_as(ctypes.c_void_p))
        return x0.value, inv.value, v

    def lj_table(self):
        """(x0, invDx, padded samples) of the -I table as the host hands it to AllocateGpu: n + 4 entries (leading pad, n + 1 samples from x0 to
        the cutoff, one more past it, trailing pad).  None without -I."""
        import numpy as np
        x0, inv = ctypes.c_double(), ctypes.c_double()
        n = self.lib.comdLjTable(self.ptr, ctypes.byref(x0), ctypes.byref(inv), None)
        if n == 0:
            return None
        v = np.empty(n + 4)
        self.lib.comdLjTable(self.ptr, ctypes.byref(x0), ctypes.byref(inv), v.ctypes.data_as(ctypes.c_void_p))
        return x0.value, inv.value, v

    # --- Langevin thermostat (not in the reference: comd-hip --langevin, --langevinTemp, --langevinDamp, --seed) ---
    def set_langevin(self, temperature, damp_fs=100.0, seed=None, on=True):
        """BAOAB Langevin thermostat from the next step() on: target `temperature` in K, damping time `damp_fs` in fs, Philox key `seed` (None:
        keep the current one, the --seed value or its default).  on=False: plain NVE again (the settings are kept)."""
        if seed is None:
            seed = self.langevin()["seed"]
        if self.lib.comdSetLangevin(self.ptr, float(temperature), float(damp_fs), int(seed) & (2 ** 64 - 1), 1 if on else 0) != 0:
            raise ValueError(f"set_langevin: need temperature >= 0 and damp_fs > 0 (got {temperature}, {damp_fs})")

    def langevin(self):
        """The thermostat settings: {"on", "temperature" (K), "damp_fs", "seed"}."""
        out, seed = (ctypes.c_double * 2)(), ctypes.c_uint64(0)
        on = self.lib.comdGetLangevin(self.ptr, out, ctypes.byref(seed))
        return {"on": bool(on), "temperature": out[0], "damp_fs": out[1], "seed": int(seed.value)}

    @property
    def step_count(self):
        """Steps taken since creation, over all step() calls: the step index of the thermostat's noise."""
        return int(self.lib.comdStepCount(self.ptr))

    @property
    def nl_builds(self):
        """Verlet-list builds so far (thread_atom_nl)."""
        return self.lib.comdNeighborListBuilds(self.ptr)

    def kinetic_energy(self):
        self.lib.kineticEnergyGpu(self.ptr)

    def sum_atoms(self):
        self.lib.sumAtoms(self.ptr)

    # --- device-side timing of the force launches (comd_hip.h comdForceTiming*, per simulation) ---
    def force_timing(self, on):
        hip = lib_hip()
        gpu = ctypes.c_void_p(self.lib.comdSimGpu(self.ptr))
        hip.comdForceTimingEnable(gpu, 1 if on else 0)
        if on:
            hip.comdForceTimingReset(gpu)

    def force_timing_total(self):
        """(milliseconds, launches) of the force kernels since force_timing(True)."""
        n = ctypes.c_int(0)
        ms = lib_hip().comdForceTimingTotalMs(ctypes.c_void_p(self.lib.comdSimGpu(self.ptr)), ctypes.byref(n))
        return ms, int(n.value)

    def force_timing_aux(self):
        """(milliseconds, launches) of what the force evaluations launched beside the force kernels (list builds, cell marks)."""
        n = ctypes.c_int(0)
        ms = lib_hip().comdForceTimingAuxMs(ctypes.c_void_p(self.lib.comdSimGpu(self.ptr)), ctypes.byref(n))
        return ms, int(n.value)

    def force_path_info(self):
        """What the force wrappers decided: LJ candidate lists in use, records of the EAM brick image, Verlet-list format, bricks in the thread-per-atom fall-back."""
        hip = lib_hip()
        gpu = ctypes.c_void_p(self.lib.comdSimGpu(self.ptr))
        a, b = (ctypes.c_int * 4)(), (ctypes.c_int * 3)()
        hip.comdForcePathInfo(gpu, a)
        hip.comdEamBrickStats(gpu, b)
        return {"lj_candidate_lists_active": bool(a[0]), "eam_brick_image_records": a[1], "neighbor_list_format": a[2], "eam_brick_cells": a[3] & 255, "eam_brick_lists_made": a[3] >> 8,
                "eam_bricks_in_thread_per_atom_fallback": b[0], "eam_bricks_per_launch": b[1]}

    def overlap_cell_counts(self):
        """The cell lists the overlap mode (-a 1) launches over, as the host built them for this grid: {"boundary" (local cells within two rings of the
        surface), "interior" (the other local cells), "boundary_ring1" (local cells that touch the halo)}.  Host state; launches nothing."""
        out = (ctypes.c_int * 3)()
        lib_hip().comdOverlapCellCounts(ctypes.c_void_p(self.lib.comdSimGpu(self.ptr)), out)
        return {"boundary": out[0], "interior": out[1], "boundary_ring1": out[2]}

    _LJ_CTA_FORMS = {0: None, 1: "boxes", 2: "slabs", 3: "pairlist"}
    _EAM_KERNELS = {0: None, 1: "brick", 2: "atom_brick", 3: "cta_cell_round2", 4: "listed_rows", 5: "nl_lds", 6: "thread_atom_round2", 7: "nl_global"}
    _EAM_COVERS = {0: "all_cells", 1: "whole_bricks", 2: "cell_by_cell"}

    def force_leg_report(self):
        """What the LAST force evaluation of this simulation ran (comd_hip.h comdForceLegReport): the wrappers' records of their launches and counts taken from the
        device arrays they fill.  Waits for the device; launches and clears nothing.  eam_bricks_streamed_total counts since creation: take the difference of two reports."""
        out = (ctypes.c_int * 32)()
        lib_hip().comdForceLegReport(ctypes.c_void_p(self.lib.comdSimGpu(self.ptr)), out)
        return {"lj_waves_per_cell": out[0], "lj_list_row_capacity": out[1], "lj_lists_active": bool(out[2]), "lj_waves_listed": out[3], "lj_waves_walking": out[4],
                "lj_candidates_min": out[5], "lj_candidates_max": out[6], "lj_cta_form": self._LJ_CTA_FORMS[out[7]],
                "eam_kernel": self._EAM_KERNELS[out[8]], "eam_brick_shape": (out[9], out[10]), "eam_image_records": out[11], "eam_bricks": out[12],
                "eam_pass1_workgroups": out[13], "eam_bricks_streamed_total": out[14], "eam_row_capacity": out[15], "eam_pass3_read_rows": bool(out[16]),
                "eam_cover": self._EAM_COVERS[out[17]], "eam_byte_offset_limit": out[18], "eam_tables_in_lds": bool(out[19]), "eam_spline": bool(out[20]),
                "eam_clamps_kept": bool(out[21]), "eam_stencil_records": out[22], "neighbor_list_format": out[23], "lj_prefetch": bool(out[24]),
                "lj_full_waves_listed": out[25], "lj_full_rows_not_multiple_of_64": out[26], "lj_full_rows_own_part_not_multiple_of_8": out[27],
                "lj_full_rows_min": out[28], "lj_prefetch_distance": out[29], "nl_row_capacity": out[30], "nl_longest_row": out[31]}

    # --- results ---
    def energy(self):
        """(ePotential, eKinetic, nGlobal) totals in eV."""
        out = (ctypes.c_double * 3)()
        self.lib.comdGetEnergy(self.ptr, out)
        return out[0], out[1], int(out[2])

    def virial(self):
        """(W, K): the global pair virial sum_{i<j} r_ij f_ij^T and kinetic tensor sum_i p_i p_i^T / m_i of the current state, 3x3 float64 in eV.
        Computed on the device from the current positions, momenta and (EAM) F'(rhobar) by computeVirial; the reference has no counterpart."""
        np = self._np
        out = (ctypes.c_double * 13)()
        self.lib.comdVirial(self.ptr, out)
        self._volume = out[12]

        def sym(c):
            xx, yy, zz, yz, xz, xy = c
            return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=np.float64)
        return sym(out[0:6]), sym(out[6:12])

    def virial_fdotr(self):
        """(W, K) like virial(), from the forces of the last force evaluation: sum_i r_i F_i^T over the atoms minus the shift term of the pairs that cross
        a periodic face (computeVirialFdotr; hip/fdotr_kernels.h has the identity).  What the barostat reads inside the step loop: a surface-sized share of
        virial()'s pair walk.  Valid after step(), set_box() or any complete force evaluation; same tensor as virial() up to rounding."""
        if self.host_only:
            raise RuntimeError("virial_fdotr: a host-only simulation has no device state")
        np = self._np
        out = (ctypes.c_double * 13)()
        self.lib.comdVirialFdotr(self.ptr, out)

        def sym(c):
            xx, yy, zz, yz, xz, xy = c
            return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=np.float64)
        return sym(out[0:6]), sym(out[6:12])

    def periodic_face_pairs(self):
        """int32 (n, 5): the work list of virial_fdotr()'s face kernel on this rank: (local cell, halo cell that holds periodic images, sign x, sign y, sign z),
        the images stored at home position + sign_a L_a.  Built from the static neighbour table and the process grid; works on a host-only simulation."""
        np = self._np
        n = self.lib.comdPeriodicFacePairs(self.ptr, None, 0)
        out = np.zeros((n, 5), dtype=np.int32)
        if n:
            self.lib.comdPeriodicFacePairs(self.ptr, out.ctypes.data_as(c_int_p), n)
        return out

    def set_barostat(self, pressure_gpa=0.0, tau_fs=1000.0, modulus_gpa=140.0, every=10, axes="xyz", iso=False, on=True):
        """Berendsen barostat for the coming step() calls: after every `every`-th step (counted by the global step) the pressure of virial_fdotr() gives
        mu_a = berendsen_scale(...) with dt_coupling = every * dt, and the next step's remap sets L_a mu_a on the axes of `axes` (a subset of "xyz").  The
        target is a scalar or (x, y, z) in GPa, compressive positive; iso=True: one mu from the mean over the chosen axes.  on=False switches it off.  With
        set_langevin() this is NPT.  ValueError, state unchanged, for what is refused: profile mode -s, an axis that also has a strain rate, every < 1, no
        axis, tau <= 0, modulus <= 0, every * dt > tau, a non-finite value.  RuntimeError on a host-only simulation."""
        if self.host_only:
            raise RuntimeError("set_barostat: a host-only simulation has no integrator")
        np = self._np
        ax = str(axes)
        mask = sum(1 << "xyz".index(c) for c in set(ax) if c in "xyz")
        if not on:
            self.lib.comdSetBarostat(self.ptr, 0, None, 0.0, 0.0, 0, 0, 0)
            return
        if len(set(ax)) != len(ax) or any(c not in "xyz" for c in ax) or not ax:
            raise ValueError(f"set_barostat: axes must be a non-empty subset of 'xyz' (got {axes!r})")
        t = np.asarray(pressure_gpa, dtype=np.float64)
        if t.shape not in ((), (3,)):
            raise ValueError(f"set_barostat: the pressure is a scalar or (x, y, z) in GPa (got {pressure_gpa!r})")
        t = np.ascontiguousarray(np.broadcast_to(t, (3,)))
        if self.lib.comdSetBarostat(self.ptr, 1, t.ctypes.data_as(c_double_p), float(tau_fs), float(modulus_gpa), int(every), mask, int(bool(iso))) != 0:
            raise ValueError(f"set_barostat: refused (pressure {t.tolist()} GPa, tau {tau_fs} fs, modulus {modulus_gpa} GPa, every {every}, axes {axes!r}): "
                             "profile mode, an axis with a strain rate, every < 1, tau <= 0, modulus <= 0, every * dt > tau or a non-finite value")

    @property
    def barostat(self):
        """The barostat's settings: {"on", "pressure_gpa" (3,), "tau_fs", "modulus_gpa", "every", "axes", "iso"}."""
        out = (ctypes.c_double * 8)()
        on = self.lib.comdGetBarostat(self.ptr, out)
        mask = int(out[6])
        return {"on": bool(on), "pressure_gpa": self._np.array(out[0:3], dtype=self._np.float64), "tau_fs": out[3], "modulus_gpa": out[4],
                "every": int(out[5]), "axes": "".join(c for a, c in enumerate("xyz") if mask >> a & 1), "iso": bool(int(out[7]))}

    # --- slab profiles and the Mueller-Plathe exchange (not in the reference: comd-hip --profile, --prof*, --mp, --mp*) ---
    _MP_WHY = {1: "axis must be 'x', 'y' or 'z'", 2: "n_bins must be even and lie in 4..1024", 3: "every must be >= 1", 4: "swaps must lie in 1..64"}

    def _slab_axis(self, what, axis, n_bins, mp=False, every=1, swaps=1):
        """the axis index, after the refusals that come before any launch"""
        if self.host_only:
            raise RuntimeError(f"{what}: a host-only simulation has no device state")
        a = "xyz".find(axis) if isinstance(axis, str) and len(axis) == 1 else -1
        if a < 0:
            raise ValueError(f"{what}: axis must be 'x', 'y' or 'z' (got {axis!r})")
        if not 1 <= int(n_bins) <= 1024:
            raise ValueError(f"{what}: n_bins must lie in 1..1024 (got {n_bins})")
        if mp:
            why = self.lib.comdMullerPlatheRefusal(a, int(n_bins), int(every), int(swaps))
            if why:
                raise ValueError(f"{what}: {self._MP_WHY[why]} (got axis {axis!r}, n_bins {n_bins}, every {every}, swaps {swaps})")
        return a

    def slab_profile(self, axis="x", n_bins=20, raw=False):
        """Profiles of the current state along `axis` in n_bins slabs of the global box, 1 <= n_bins <= 1024: {"edges" float64 (n + 1,) in Angstroms, "count" int64,
        "momentum" (n, 3) the sum of p in eV fs/A, "kinetic" the sum of |p|^2 / 2m and "potential" the sum of the per-atom energies in eV, "temperature"
        2 kinetic / (3 kB count) in K, NaN where the slab is empty}.  An atom at r is in bin int(floor(r * invWidth)) mod n_bins with invWidth = n_bins / L in the
        build's precision.  Summed on the device in 64-bit integers (computeSlabProfile: units of 2^-32, every atom's term rounded once) and over the ranks, so the
        result is the same bits for every method, cell order and rank count; raw=True adds "raw", the int64 (6, n) planes count, p_x, p_y, p_z, KE, e.  The energies
        are current after creation, compute_force(), set_box() and between step() calls.  ValueError for a bad axis or n_bins, RuntimeError on a host-only simulation."""
        np = self._np
        a = self._slab_axis("slab_profile", axis, n_bins)
        n = int(n_bins)
        planes = np.zeros((6, n), dtype=np.int64)
        if self.lib.comdSlabProfile(self.ptr, a, n, planes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) != 0:
            raise RuntimeError("slab_profile: comdSlabProfile failed")
        unit = 1.0 / 4294967296.0
        count = planes[0].copy()
        kinetic = planes[4] * unit
        with np.errstate(divide="ignore", invalid="ignore"):
            temperature = np.where(count > 0, 2.0 * kinetic / (3.0 * 8.6173324e-5 * count), np.nan)
        out = {"edges": np.arange(n + 1, dtype=np.float64) * (self.box[a] / n), "count": count, "momentum": np.ascontiguousarray(planes[1:4].T * unit),
               "kinetic": kinetic, "potential": planes[5] * unit, "temperature": temperature}
        if raw:
            out["raw"] = planes
        return out

    def muller_plathe_table(self, axis="x", n_bins=20, swaps=1):
        """(cold, hot): float64 (nRanks * swaps, 6) each, the candidate table of comdMullerPlatheCandidates as every rank receives it: rank r's rows r * swaps ..., each
        rank's rows in the pick order of the device (MP_select, MP_merge), a row {KE, gid + 1, p_x, p_y, p_z, slot on its rank}, a row of zeros empty.  What
        muller_plathe_candidates() takes its global lists from (comdMullerPlatheTop) and muller_plathe_match() accepts.  Refusals as muller_plathe_candidates."""
        return self._mp_table(self._slab_axis("muller_plathe_table", axis, n_bins, True, 1, swaps), n_bins, swaps)

    def _mp_table(self, a, n_bins, swaps):
        """the candidate rows of all ranks: (cold (nRanks * k, 6), hot (nRanks * k, 6)) of comdMullerPlatheCandidates"""
        np = self._np
        k, world = int(swaps), self.lib.getNRanks()
        table = np.zeros((2, world * k, 6), dtype=np.float64)
        if self.lib.comdMullerPlatheCandidates(self.ptr, a, int(n_bins), k, table.ctypes.data_as(c_double_p)) != 0:
            raise RuntimeError("muller_plathe_candidates: comdMullerPlatheCandidates failed")
        return table[0], table[1]

    def muller_plathe_candidates(self, axis="x", n_bins=20, swaps=1):
        """{"cold_hottest": (gids int64, ke float64), "hot_coldest": (gids, ke)}: the `swaps` atoms of largest kinetic energy in slab 0 and of smallest in slab
        n_bins / 2 of slab_profile()'s slabs, global, in pick order -- by (KE, gid), the lower gid first among equal KE -- fewer where a slab holds fewer atoms.
        Selected on the device (computeMullerPlatheCandidates) and merged over the ranks in the C routine the exchange itself uses (comdMullerPlatheTop); changes nothing.  ValueError for a bad axis, an odd n_bins or one
        outside 4..1024, swaps outside 1..64."""
        np = self._np
        a = self._slab_axis("muller_plathe_candidates", axis, n_bins, True, 1, swaps)
        out = {}
        for name, rows, hot in zip(("cold_hottest", "hot_coldest"), self._mp_table(a, n_bins, swaps), (False, True)):
            rows = np.ascontiguousarray(rows)
            top = np.zeros(int(swaps), dtype=np.int32)
            n = self.lib.comdMullerPlatheTop(rows.ctypes.data_as(c_double_p), rows.shape[0], int(swaps), int(hot), top.ctypes.data_as(c_int_p))
            out[name] = ((rows[top[:n], 1] - 1.0).astype(np.int64), rows[top[:n], 0].copy())
        return out

    def muller_plathe_swap(self, axis="x", n_bins=20, swaps=1):
        """One Mueller-Plathe exchange on the current state: the j-th hottest atom of slab 0 and the j-th coldest of slab n_bins / 2 swap their momentum vectors bit
        for bit, j < swaps, as long as the first is hotter than the second (from the first pair that is not, all are skipped).  Returns (pairs int64 (n, 2) of
        gids (cold-slab atom, hot-slab atom), delta_e in eV carried to the hot slab, skipped = swaps - n).  Positions, forces and every other momentum stay; the
        tally of `muller_plathe` grows.  Every rank of a multi-rank run makes the call.  ValueError as muller_plathe_candidates."""
        np = self._np
        a = self._slab_axis("muller_plathe_swap", axis, n_bins, True, 1, swaps)
        pairs = np.zeros((int(swaps), 2), dtype=np.int32)
        d_e, skipped = ctypes.c_double(0.0), ctypes.c_int(0)
        kept = self.lib.comdMullerPlatheSwap(self.ptr, a, int(n_bins), int(swaps), pairs.ctypes.data_as(c_int_p), ctypes.byref(d_e), ctypes.byref(skipped))
        if kept < 0:
            raise RuntimeError("muller_plathe_swap: comdMullerPlatheSwap failed")
        return pairs[:kept].astype(np.int64), d_e.value, int(skipped.value)

    def set_muller_plathe(self, axis="x", n_bins=20, every=100, swaps=1, start=None, on=True):
        """The exchange inside the coming step() calls: at the end of every step whose global count c satisfies c > start and (c - start) % every == 0 (start None: the
        current step count) the step ends unfused and muller_plathe_swap(axis, n_bins, swaps) runs behind its closing half kick, so step(3); step(7) exchanges
        where step(10) does.  on=False switches it off (the tally stays).  ValueError, state unchanged, as muller_plathe_candidates, for every < 1 or start < 0."""
        if not on:
            if self.host_only:
                raise RuntimeError("set_muller_plathe: a host-only simulation has no integrator")
            self.lib.comdSetMullerPlathe(self.ptr, 0, 0, 0, 0, 0, 0)
            return
        a = self._slab_axis("set_muller_plathe", axis, n_bins, True, every, swaps)
        start = self.step_count if start is None else int(start)
        if start < 0 or self.lib.comdSetMullerPlathe(self.ptr, 1, a, int(n_bins), int(every), int(swaps), start) != 0:
            raise ValueError(f"set_muller_plathe: refused (axis {axis!r}, n_bins {n_bins}, every {every}, swaps {swaps}, start {start})")

    @property
    def muller_plathe(self):
        """The exchange's settings and tally: {"on", "axis", "n_bins", "every", "swaps", "start", "exchanged_ev", "pairs", "skipped"}."""
        out = (ctypes.c_double * 8)()
        on = self.lib.comdGetMullerPlathe(self.ptr, out)
        return {"on": bool(on), "axis": "xyz"[int(out[0])], "n_bins": int(out[1]), "every": int(out[2]), "swaps": int(out[3]), "start": int(out[4]),
                "exchanged_ev": out[5], "pairs": int(out[6]), "skipped": int(out[7])}

    # --- static structure factor and Bragg order (not in the reference: comd-hip --sk, --skStride, --skBins, --skStart, --skFile) ---
    def structure_factor(self, k_max=8, stride=1):
        """The static structure factor of the current state on the half grid of wave vectors k = 2 pi (sx h / Lx, sy k / Ly, sz l / Lz), h in [0, k_max], k, l in
        [-k_max, k_max] (S(-k) = S(k)), on the current box: {"index" int32 (K, 3) the (h, k, l), "k" float64 (K, 3) in 1/Angstrom, "rho" complex128 (K,) the density
        amplitudes sum_j exp(-i k . r_j) over the atoms of all ranks, "s" float64 (K,) = |rho|^2 / N, "shape" (k_max + 1, 2 k_max + 1, 2 k_max + 1) the C order of
        the K rows}; (0, 0, 0) is kept and its rho is N exactly.  `stride` is an int or (sx, sy, sz): with the unit cells of -x -y -z the grid is the reciprocal
        lattice of the conventional cubic cell, where a perfect FCC crystal has S = N for h, k, l all even or all odd and 0 elsewhere.  1 <= k_max <= 64, strides
        >= 1 with stride k_max <= 65536.  Summed on the device by computeStructureFactor and over the ranks (every rank gets the global result).  Each amplitude
        component is within N eps (16 + 2 pi max|stride index|) of the exact sum, eps that of the build's real type; one configuration gives the same bits at every
        call, but methods, cell orders and rank counts add the atoms in different orders and differ within that bound.  ValueError before anything is launched
        for a refused grid, RuntimeError on a host-only simulation."""
        np = self._np
        m, st = _sk_grid("structure_factor", k_max, stride)
        if self.host_only:
            raise RuntimeError("structure_factor: a host-only simulation has no device state")
        w = 2 * m + 1
        raw = np.zeros(((m + 1) * w * w, 2), dtype=np.float64)
        if self.lib.comdStructureFactor(self.ptr, m, st.ctypes.data_as(c_int_p), raw.ctypes.data_as(c_double_p)) != 0:
            raise RuntimeError("structure_factor: comdStructureFactor failed")
        index = _sk_index(np, m)
        rho = raw[:, 0] + 1j * raw[:, 1]
        return {"index": index, "k": 2.0 * np.pi * (index * st[None, :]) / self.box[None, :], "rho": rho, "s": (raw[:, 0] ** 2 + raw[:, 1] ** 2) / float(self.n_global),
                "shape": (m + 1, w, w)}

    def structure_factor_radial(self, k_max=8, stride=1, n_bins=50):
        """(k centres in 1/Angstrom, S, counts): the powder average of structure_factor(k_max, stride) in n_bins uniform |k| bins up to the largest sphere inside
        the grid -- the module function structure_factor_radial() on this state's amplitudes and box."""
        _sk_grid("structure_factor_radial", k_max, stride)
        if not 1 <= int(n_bins) <= 4096:
            raise ValueError(f"structure_factor_radial: n_bins must lie in 1..4096 (got {n_bins})")
        return structure_factor_radial(self.structure_factor(k_max, stride)["rho"], k_max, stride, self.box, n_bins)

    def bragg_order(self):
        """The Bragg order parameter: the mean over the reflections (1, +-1, +-1) of S / N at the strides (nx, ny, nz) of -x -y -z -- the {111} peaks of the
        conventional cell.  1 on the perfect lattice, the Debye-Waller factor of a warm crystal, of the order 1/N in the melt; the indices follow the box, so an
        affine strain leaves it at 1.  One comdStructureFactor call with k_max = 1.  RuntimeError on a host-only simulation."""
        if self.host_only:
            raise RuntimeError("bragg_order: a host-only simulation has no device state")
        out = ctypes.c_double(0.0)
        if self.lib.comdBraggOrder(self.ptr, ctypes.byref(out)) != 0:
            raise RuntimeError("bragg_order: comdBraggOrder failed")
        return out.value

    def pressure_tensor(self):
        """(K + W) / V in eV/A^3, V the volume of the global domain (positive: compressive).  1 eV/A^3 = 160.21766208 GPa."""
        w, k = self.virial()
        return (k + w) / self._volume

    def pressure(self):
        """trace(pressure_tensor()) / 3 in eV/A^3."""
        return float(self._np.trace(self.pressure_tensor())) / 3.0

    # --- structure (not in the reference: comd-hip --rdf, --rdfMax, --rdfFile) ---
    @property
    def cutoff(self):
        """The force cutoff of the potential in use, in Angstroms."""
        return self.lib.comdCutoff(self.ptr)

    def pair_histogram(self, n_bins, r_max=None):
        """(edges float64[n_bins + 1], counts int64[n_bins]): the global number of unordered pairs of the current state in n_bins uniform bins
        [k dr, (k + 1) dr) up to r_max Angstroms (None: the force cutoff, which is also the most it can be); 1 <= n_bins <= 4096.  Counted on the
        device by computePairHistogram, summed over the ranks (every rank gets the global result); valid whenever virial() is."""
        np = self._np
        n_bins = int(n_bins)
        out = np.zeros(max(n_bins, 1), dtype=np.float64)
        # r_max <= 0 means "the cutoff" to comdPairHistogram: refuse it here, before anything is launched
        if (r_max is not None and not r_max > 0.0) \
                or self.lib.comdPairHistogram(self.ptr, n_bins, 0.0 if r_max is None else float(r_max), out.ctypes.data_as(c_double_p)) != 0:
            raise ValueError(f"pair_histogram: need 1 <= n_bins <= 4096 and 0 < r_max <= the force cutoff {self.cutoff} (got {n_bins}, {r_max})")
        edges = np.arange(n_bins + 1, dtype=np.float64) * ((self.cutoff if r_max is None else float(r_max)) / n_bins)
        return edges, _whole_pairs(np, out)

    def rdf(self, n_bins, r_max=None):
        """(r_centres, g): the radial distribution function g_k = counts_k / ((N/2) (N/V) (4 pi/3) ((k + 1)^3 - k^3) dr^3) of pair_histogram's bins."""
        np = self._np
        edges, counts = self.pair_histogram(n_bins, r_max)
        n, dr = float(self.n_global), edges[-1] / n_bins
        k = np.arange(n_bins, dtype=np.float64)
        ideal = (0.5 * n) * (n / self.lib.comdVolume(self.ptr)) * (4.0 * np.pi / 3.0 * dr * dr * dr) * ((k + 1.0) ** 3 - k ** 3)
        return 0.5 * (edges[:-1] + edges[1:]), counts / ideal

    # --- defects (not in the reference: comd-hip --csp, --cspThreshold, --cspCoord, --cspFile, --cspDump) ---
    @property
    def lattice_constant(self):
        """The lattice constant the crystal was made with (-l, or the potential's), in Angstroms."""
        return self.lib.comdLatticeConstant(self.ptr)

    def centro_symmetry(self, r_coord=None):
        """(csp float64[n_global], coordination int32[n_global]) of the current state, keyed by gid.  csp: the centro-symmetry parameter in
        Angstroms^2, the sum in ascending order of the 6 smallest |R_a + R_b|^2 over the 66 pairs of the offset vectors of the atom's 12 nearest
        neighbours -- 0 on a perfect FCC site, 24 |d|^2 for an atom displaced alone by d, lat^2 / 2 in a stacking fault, +inf with fewer than 12
        neighbours inside the force cutoff.  coordination: the neighbours closer than r_coord Angstroms (None: halfway between the first and second
        FCC shells, (1/sqrt 2 + 1) lat / 2, or the force cutoff where that is smaller; at most the force cutoff).  Computed on the device by
        computeCentroSymmetry, summed over the ranks (every rank gets the global arrays); valid whenever pair_histogram() is."""
        np = self._np
        if self.host_only:
            raise RuntimeError("centro_symmetry: a host-only simulation has no device state")
        # r_coord <= 0 means "the default" to comdCentroSymmetry: refuse it here, before anything is launched
        if r_coord is not None and not (0.0 < float(r_coord) <= self.cutoff):
            raise ValueError(f"centro_symmetry: need 0 < r_coord <= the force cutoff {self.cutoff} (got {r_coord})")
        n = self.n_global
        csp, coord = np.zeros(max(n, 1), dtype=np.float64), np.zeros(max(n, 1), dtype=np.float64)
        if self.lib.comdCentroSymmetry(self.ptr, 0.0 if r_coord is None else float(r_coord), csp.ctypes.data_as(c_double_p), coord.ctypes.data_as(c_double_p)) != 0:
            raise ValueError(f"centro_symmetry: r_coord {r_coord} was refused (the force cutoff is {self.cutoff})")
        return csp[:n], coord[:n].astype(np.int32)

    def defects(self, threshold=None, r_coord=None):
        """Ascending int64 gids of the atoms whose centro-symmetry parameter exceeds `threshold` Angstroms^2 (None: lat^2 / 4, half the value of an
        atom in a stacking fault); atoms with fewer than 12 neighbours (+inf) count."""
        np = self._np
        if self.host_only:
            raise RuntimeError("defects: a host-only simulation has no device state")
        if threshold is not None and not float(threshold) > 0.0:
            raise ValueError(f"defects: need threshold > 0 (got {threshold})")
        if threshold is None:
            threshold = 0.25 * self.lattice_constant ** 2
        csp, _ = self.centro_symmetry(r_coord)
        return np.nonzero(csp > float(threshold))[0].astype(np.int64)

    # --- structure identification (not in the reference: comd-hip --cna, --cnaFile, --cnaDump) ---
    def _cna(self, what):
        np = self._np
        if self.host_only:
            raise RuntimeError(f"{what}: a host-only simulation has no device state")
        n = self.n_global
        types, counts = np.zeros(max(n, 1), dtype=np.int32), (ctypes.c_longlong * 5)()
        if self.lib.comdCommonNeighbors(self.ptr, types.ctypes.data_as(c_int_p), counts) != 0:
            raise RuntimeError(f"{what}: comdCommonNeighbors failed")
        return types[:n], counts

    def common_neighbor_analysis(self):
        """int32[n_global] keyed by gid: the structure every atom of the current state sits in, by adaptive common neighbour analysis (Stukowski 2012)
        on its 12 nearest neighbours inside the force cutoff -- CNA_FCC (1), CNA_HCP (2), CNA_ICO (4), CNA_OTHER (0) for everything else, atoms with
        fewer than 12 such neighbours included; OVITO's numbers, 3 (BCC) is never returned.  Computed on the device by computeCommonNeighbors, summed
        over the ranks (every rank gets the global array); valid whenever centro_symmetry() is."""
        return self._cna("common_neighbor_analysis")[0]

    def structure_counts(self):
        """{"other", "fcc", "hcp", "ico"}: how many atoms common_neighbor_analysis() gives each type."""
        counts = self._cna("structure_counts")[1]
        return {"other": int(counts[CNA_OTHER]), "fcc": int(counts[CNA_FCC]), "hcp": int(counts[CNA_HCP]), "ico": int(counts[CNA_ICO])}

    # --- per-atom stress (not in the reference: comd-hip --stress, --stressFile, --stressDump, --stressDumpMin) ---
    @property
    def atomic_volume(self):
        """The uniform atomic volume V / N of the current box in Angstroms^3 (no Voronoi volumes)."""
        return self.volume / self.n_global

    def atomic_stress(self, kinetic=True):
        """float64 (n_global, 6) keyed by gid: every atom's virial stress x volume in eV, tension positive, components xx yy zz yz xz xy,
        s_i = -([kinetic] p_i p_i^T / m_i + 1/2 sum_j r_ij f_ij^T) over the neighbours inside the force cutoff, with the pair convention of virial():
        the rows add up to -(K + W), or -W without the kinetic term.  Computed on the device by computeAtomStress, summed over the ranks (every
        rank gets the global array); valid whenever virial() is."""
        np = self._np
        if self.host_only:
            raise RuntimeError("atomic_stress: a host-only simulation has no device state")
        n = self.n_global
        out = np.zeros((max(n, 1), 6), dtype=np.float64)
        if self.lib.comdAtomStress(self.ptr, 1 if kinetic else 0, out.ctypes.data_as(c_double_p)) != 0:
            raise RuntimeError("atomic_stress: comdAtomStress failed")
        return out[:n]

    def atomic_pressure(self, kinetic=True):
        """float64 (n_global,): the hydrostatic pressure -(s_xx + s_yy + s_zz) / (3 atomic_volume) of atomic_stress(), in eV/A^3 (x GPA_PER_EV_A3 = GPa)."""
        s = self.atomic_stress(kinetic)
        return -((s[:, 0] + s[:, 1]) + s[:, 2]) * ((1.0 / self.atomic_volume) / 3.0)

    def von_mises(self, kinetic=True):
        """float64 (n_global,): the von Mises stress sqrt(1/2 [(s_xx - s_yy)^2 + (s_yy - s_zz)^2 + (s_zz - s_xx)^2] + 3 (s_yz^2 + s_xz^2 + s_xy^2)) / atomic_volume
        of atomic_stress(), in eV/A^3."""
        np = self._np
        s = self.atomic_stress(kinetic)
        d0, d1, d2 = s[:, 0] - s[:, 1], s[:, 1] - s[:, 2], s[:, 2] - s[:, 0]
        return np.sqrt(0.5 * ((d0 * d0 + d1 * d1) + d2 * d2) + 3.0 * ((s[:, 3] * s[:, 3] + s[:, 4] * s[:, 4]) + s[:, 5] * s[:, 5])) * (1.0 / self.atomic_volume)

    def stress_summary(self, kinetic=True):
        """{"mean_pressure", "min_pressure", "max_pressure", "mean_von_mises", "max_von_mises", "max_von_mises_gid", "n"}: the figures of atomic_pressure()
        and von_mises() in eV/A^3, reduced on the device (computeAtomStressSummary: the per-atom planes never leave it) and over the ranks; the gid is the
        lowest one that holds the maximum."""
        if self.host_only:
            raise RuntimeError("stress_summary: a host-only simulation has no device state")
        out = (ctypes.c_double * 7)()
        if self.lib.comdStressSummary(self.ptr, 1 if kinetic else 0, out) != 0:
            raise RuntimeError("stress_summary: comdStressSummary failed")
        return {"mean_pressure": out[0], "min_pressure": out[1], "max_pressure": out[2], "mean_von_mises": out[3], "max_von_mises": out[4],
                "max_von_mises_gid": int(out[5]), "n": int(out[6])}

    # --- heat flux (not in the reference: comd-hip --heatflux, --hfStart, --hfWindow, --hfFile, --hfAcfFile) ---
    @property
    def mass(self):
        """The mass of the (one) species in eV fs^2/A^2: v = p / mass."""
        return self.lib.comdAtomMass(self.ptr)

    def heat_flux(self):
        """{"kinetic", "potential", "virial", "total"}: float64 (3,) each, the heat flux J V of the current state in eV A/fs (flux density x volume), summed
        over all atoms of all ranks on the device (computeHeatFlux; nothing per atom leaves it): sum_i (|p_i|^2 / 2 m) v_i, sum_i e_i v_i,
        1/2 sum_i sum_j r_ij (f_ij . v_i), and their sum.  Valid when virial() is and the per-atom energies are current: after creation, compute_force(),
        set_box() or a step() call -- between step() calls, whose last step evaluates the energies."""
        np = self._np
        if self.host_only:
            raise RuntimeError("heat_flux: a host-only simulation has no device state")
        out = (ctypes.c_double * 9)()
        if self.lib.comdHeatFlux(self.ptr, out) != 0:
            raise RuntimeError("heat_flux: comdHeatFlux failed")
        j = np.array(out[0:9], dtype=np.float64)
        return {"kinetic": j[0:3].copy(), "potential": j[3:6].copy(), "virial": j[6:9].copy(), "total": (j[0:3] + j[3:6]) + j[6:9]}

    def atomic_heat_flux(self):
        """float64 (n_global, 9) keyed by gid: every atom's kinetic (columns 0-2), potential (3-5) and virial (6-8) part of heat_flux(), x y z each, in
        eV A/fs; summed over the ranks (every rank gets the global array)."""
        np = self._np
        if self.host_only:
            raise RuntimeError("atomic_heat_flux: a host-only simulation has no device state")
        n = self.n_global
        out = np.zeros((max(n, 1), 9), dtype=np.float64)
        if self.lib.comdAtomHeatFlux(self.ptr, out.ctypes.data_as(c_double_p)) != 0:
            raise RuntimeError("atomic_heat_flux: comdAtomHeatFlux failed")
        return out[:n]

    def heat_flux_density(self):
        """float64 (3,): heat_flux()["total"] / volume, the heat flux density J in eV/A^2/fs."""
        return self.heat_flux()["total"] / self.volume

    # --- per-atom strain (not in the reference: comd-hip --strain, --strainRef, --strainCutoff, --strainThreshold, --strainFile, --strainDump, --strainDumpMin) ---
    def set_strain_reference(self, on=True):
        """Take the current state as the reference of atomic_strain(): every atom's position, keyed by gid, in a table of doubles on every rank's device
        (32 bytes per global atom), and the current box.  Already set: the reference moves to the current state.  on=False drops it and frees the device
        memory.  Every rank of a multi-rank run makes the call.  RuntimeError when the device refuses the memory."""
        if self.host_only:
            raise RuntimeError("set_strain_reference: a host-only simulation has no device state")
        if self.lib.comdStrainReference(self.ptr, 1 if on else 0) != 0:
            raise RuntimeError(f"set_strain_reference: no device memory for the reference positions of {self.n_global} atoms")

    @property
    def strain_reference_box(self):
        """float64 (3,): the extents of the global box when set_strain_reference() was called.  ValueError without a reference."""
        out = (ctypes.c_double * 3)()
        if self.lib.comdStrainReferenceBox(self.ptr, out) != 0:
            raise ValueError("strain_reference_box: no reference (call set_strain_reference() first)")
        return self._np.array(out[0:3], dtype=self._np.float64)

    def _strain_cutoff(self, what, cutoff):
        """the radius handed to the host (0 = its default), after the refusals that come before any launch"""
        if self.host_only:
            raise RuntimeError(f"{what}: a host-only simulation has no device state")
        if self.lib.comdStrainReferenceBox(self.ptr, (ctypes.c_double * 3)()) != 0:
            raise ValueError(f"{what}: no reference (call set_strain_reference() first)")
        if cutoff is not None and not (0.0 < float(cutoff) <= self.cutoff):
            raise ValueError(f"{what}: need 0 < cutoff <= the force cutoff {self.cutoff} (got {cutoff})")
        return 0.0 if cutoff is None else float(cutoff)

    def atomic_strain(self, cutoff=None):
        """(E float64 (n_global, 6), d2min float64 (n_global,), neighbours int32 (n_global,)) of the current state against the reference, keyed by gid.
        For atom i with its neighbours j within `cutoff` Angstroms in the CURRENT configuration (None: halfway between the first two FCC shells, as
        centro_symmetry's r_coord; at most the force cutoff), d = x_j - x_i now and d0 the same separation in the reference (minimum image of the reference
        box): F = (sum d d0^T)(sum d0 d0^T)^-1 is the best affine map d ~ F d0, E = 1/2 (F^T F - I) the Green-Lagrange strain, components xx yy zz yz xz xy,
        and d2min = sum_j |d - F d0|^2 in Angstroms^2 the non-affine residue (Falk and Langer's D^2min, not divided by the neighbour count).  An atom with
        fewer than 3 neighbours or a singular sum d0 d0^T has NaN in E and d2min.  Computed on the device by computeAtomStrain, summed over the ranks (every
        rank gets the global arrays).  ValueError, before anything is launched, without a reference or for a cutoff outside (0, force cutoff]."""
        np = self._np
        r = self._strain_cutoff("atomic_strain", cutoff)
        n = self.n_global
        out, count = np.zeros((max(n, 1), 7), dtype=np.float64), np.zeros(max(n, 1), dtype=np.int32)
        if self.lib.comdAtomStrain(self.ptr, r, out.ctypes.data_as(c_double_p), count.ctypes.data_as(c_int_p)) != 0:
            raise RuntimeError("atomic_strain: comdAtomStrain failed")
        return out[:n, :6].copy(), out[:n, 6].copy(), count[:n]

    @staticmethod
    def _shear_of(np, e):
        d0, d1, d2 = e[:, 0] - e[:, 1], e[:, 1] - e[:, 2], e[:, 2] - e[:, 0]
        return np.sqrt(((e[:, 3] * e[:, 3] + e[:, 4] * e[:, 4]) + e[:, 5] * e[:, 5]) + ((d0 * d0 + d1 * d1) + d2 * d2) / 6.0)

    def shear_strain(self, cutoff=None):
        """float64 (n_global,): the shear invariant sqrt(E_yz^2 + E_xz^2 + E_xy^2 + [(E_xx - E_yy)^2 + (E_yy - E_zz)^2 + (E_zz - E_xx)^2] / 6) of atomic_strain()."""
        return self._shear_of(self._np, self.atomic_strain(cutoff)[0])

    def volumetric_strain(self, cutoff=None):
        """float64 (n_global,): tr(E) / 3 of atomic_strain()."""
        e = self.atomic_strain(cutoff)[0]
        return ((e[:, 0] + e[:, 1]) + e[:, 2]) / 3.0

    def strain_summary(self, cutoff=None, threshold=None):
        """{"n", "invalid", "mean_shear", "max_shear", "max_shear_gid", "mean_volumetric", "mean_d2min", "max_d2min", "above_threshold"}: the figures of
        shear_strain(), volumetric_strain() and d2min, reduced on the device (computeAtomStrainSummary: the per-atom planes never leave it) and over the
        ranks.  Invalid atoms are counted and left out of means and extremes; the gid is the lowest one that holds the maximum; above_threshold counts
        the atoms with a shear strain >= threshold (None: 0.1).  With no valid atom at all (a gas: every atom has fewer than 3 neighbours) invalid == n, the means
        and extremes are 0 and max_shear_gid is -1: that is what comdStrainSummary writes for N = 0.  ValueError as atomic_strain, or for a threshold that is not > 0."""
        r = self._strain_cutoff("strain_summary", cutoff)
        if threshold is not None and not float(threshold) > 0.0:
            raise ValueError(f"strain_summary: need threshold > 0 (got {threshold})")
        out = (ctypes.c_double * 9)()
        if self.lib.comdStrainSummary(self.ptr, r, 0.1 if threshold is None else float(threshold), out) != 0:
            raise RuntimeError("strain_summary: comdStrainSummary failed")
        return {"n": int(out[0]), "invalid": int(out[1]), "mean_shear": out[2], "max_shear": out[3], "max_shear_gid": int(out[4]),
                "mean_volumetric": out[5], "mean_d2min": out[6], "max_d2min": out[7], "above_threshold": int(out[8])}

    # --- bond-orientational order (not in the reference: comd-hip --steinhardt, --stSolid, --stFile, --stDump, --stDumpMax) ---
    STEINHARDT_SOLID = 0.45

    def _steinhardt_threshold(self, what, threshold):
        """the q6 threshold handed to the host, after the refusals that come before any launch"""
        if self.host_only:
            raise RuntimeError(f"{what}: a host-only simulation has no device state")
        if threshold is not None and not (0.0 < float(threshold) < 1.0):
            raise ValueError(f"{what}: need 0 < threshold < 1 (got {threshold})")
        return self.STEINHARDT_SOLID if threshold is None else float(threshold)

    def steinhardt(self):
        """float64 (n_global, 4) keyed by gid, columns q4 q6 w4 w6: Steinhardt's bond-orientational order (Steinhardt, Nelson, Ronchetti 1983) of every atom
        of the current state on its 12 nearest neighbours inside the force cutoff, the set centro_symmetry() takes.  With the unit vectors u_ij to them,
        q_lm = (1/12) sum_j Y_lm(u_ij), q_l = sqrt(4 pi / (2l + 1) sum_m |q_lm|^2) and w_l = sum_{m1+m2+m3=0} (l l l; m1 m2 m3) q_lm1 q_lm2 q_lm3 /
        (sum_m |q_lm|^2)^(3/2): q6 is 0.575 on an FCC site, 0.485 on an HCP one, 0.663 in an icosahedron and falls continuously in a melt; w4 is negative
        for FCC and positive for HCP; w6 = -0.170 singles out the icosahedron.  w_l is 0 where q_l^2 < 1e-6.  An atom with fewer than 12 neighbours inside
        the cutoff is a NaN row.  Computed on the device by computeSteinhardt, summed over the ranks (every rank gets the global array); valid whenever
        centro_symmetry() is.  RuntimeError on a host-only simulation."""
        np = self._np
        self._steinhardt_threshold("steinhardt", None)
        n = self.n_global
        out = np.zeros((max(n, 1), 4), dtype=np.float64)
        if self.lib.comdSteinhardt(self.ptr, out.ctypes.data_as(c_double_p)) != 0:
            raise RuntimeError("steinhardt: comdSteinhardt failed")
        return out[:n]

    def steinhardt_summary(self, threshold=None):
        """{"n", "invalid", "mean_q4", "mean_q6", "min_q6", "min_q6_gid", "max_q6", "mean_w4", "mean_w6", "solid"}: the figures of steinhardt(), reduced on
        the device (computeSteinhardtSummary: the per-atom planes never leave it) and over the ranks.  n counts the valid atoms; the invalid ones are counted
        and left out of means and extremes; the gid is the lowest one that holds the minimum; solid counts the atoms with q6 >= threshold (None: 0.45).  With
        no valid atom at all invalid is the number of atoms, the means and extremes are 0 and min_q6_gid is -1.  ValueError, before anything is launched, for
        a threshold outside (0, 1); RuntimeError on a host-only simulation."""
        t = self._steinhardt_threshold("steinhardt_summary", threshold)
        out = (ctypes.c_double * 10)()
        if self.lib.comdSteinhardtSummary(self.ptr, t, out) != 0:
            raise RuntimeError("steinhardt_summary: comdSteinhardtSummary failed")
        return {"n": int(out[0]), "invalid": int(out[1]), "mean_q4": out[2], "mean_q6": out[3], "min_q6": out[4], "min_q6_gid": int(out[5]),
                "max_q6": out[6], "mean_w4": out[7], "mean_w6": out[8], "solid": int(out[9])}

    def solid_like(self, threshold=None):
        """Ascending int64 gids of the atoms with q6 >= threshold (None: 0.45); atoms with fewer than 12 neighbours (NaN) do not count.  ValueError, before
        anything is launched, for a threshold outside (0, 1)."""
        np = self._np
        t = self._steinhardt_threshold("solid_like", threshold)
        with np.errstate(invalid="ignore"):
            return np.nonzero(self.steinhardt()[:, 1] >= t)[0].astype(np.int64)

    # --- Born matrix and elastic constants (not in the reference: comd-hip --elastic, --elStart, --elFile) ---
    def born_matrix(self):
        """float64 (6, 6), symmetric, in eV: the Born matrix B_IJ = d^2 U / d eta_I d eta_J of the current state, eta the Lagrangian strain, Voigt order
        xx yy zz yz xz xy (extensive: divide by volume for a modulus).  B_abcd = sum_i [sum_j (1/2 (phi'' - phi'/r) + F'_i (rho'' - rho'/r)) r_a r_b r_c r_d / r^2
        + F''(rhobar_i) g^i_ab g^i_cd], g^i_ab = sum_j rho'(r) r_a r_b / r, over the neighbours inside the force cutoff, with the derivatives of the force
        the kernels apply.  Computed on the device by computeBornMatrix, summed over the ranks (the same on every rank); valid whenever virial() is."""
        if self.host_only:
            raise RuntimeError("born_matrix: a host-only simulation has no device state")
        np = self._np
        tri = np.zeros(21, dtype=np.float64)
        if self.lib.comdBornMatrix(self.ptr, tri.ctypes.data_as(c_double_p)) != 0:
            raise RuntimeError("born_matrix: comdBornMatrix failed")
        out = np.zeros((6, 6), dtype=np.float64)
        out[np.triu_indices(6)] = tri
        return out + np.triu(out, 1).T

    def born_constants(self):
        """{"C11", "C12", "C44"}: the cubic averages of born_matrix() / volume in eV/A^3 (x GPA_PER_EV_A3 = GPa): the elastic constants of a
        stress-free lattice at T = 0, and the Born part of elastic_constants() otherwise."""
        return _cubic_averages(self.born_matrix() / self.volume)

    # --- box deformation (not in the reference: comd-hip --erateX, --erateY, --erateZ, --deformStart, --deformFile) ---
    def _box6(self):
        out = (ctypes.c_double * 6)()
        self.lib.comdGetBox(self.ptr, out)
        return self._np.array(out[0:6], dtype=self._np.float64)

    @property
    def box(self):
        """float64 (3,): the current extents of the global box in Angstroms (its origin is 0)."""
        return self._box6()[0:3].copy()

    @property
    def box0(self):
        """float64 (3,): the extents the simulation was created with."""
        return self._box6()[3:6].copy()

    @property
    def strain(self):
        """float64 (3,): the engineering strain box / box0 - 1."""
        b = self._box6()
        return b[0:3] / b[3:6] - 1.0

    @property
    def volume(self):
        """The current volume of the global box in Angstroms^3."""
        return self.lib.comdVolume(self.ptr)

    def local_bounds(self):
        """(localMin, localMax): float64 (3,) each, this rank's brick of the global box."""
        out = (ctypes.c_double * 6)()
        self.lib.comdLocalBounds(self.ptr, out)
        return self._np.array(out[0:3], dtype=self._np.float64), self._np.array(out[3:6], dtype=self._np.float64)

    def set_box(self, extents):
        """Remap to a box of `extents` (3 lengths in Angstroms): every atom's position is scaled with the box, L_new / L_old per axis about the origin, on the
        device (momenta stay: LAMMPS's `remap x`); then the atoms are redistributed (with Verlet lists: the lists built), the forces evaluated and the
        energies read, so energy(), virial(), gather() and the analyses see the new state.  Every rank of a multi-rank run makes the call.  ValueError, state
        unchanged, for an extent that is not positive or a box whose link cells would be narrower than the interaction range the grid was built for (the
        cutoff, plus the skin with thread_atom_nl and -L).  On a host-only simulation only the host geometry changes (Domain, LinkCell, the periodic
        shifts); no atom moves."""
        np = self._np
        L = np.ascontiguousarray(np.broadcast_to(np.asarray(extents, dtype=np.float64), (3,)))
        fn = self.lib.comdSetBox if self.host_only else self.lib.comdDeformTo
        if fn(self.ptr, L.ctypes.data_as(c_double_p)) != 0:
            raise ValueError(f"set_box: extents {L.tolist()} refused: they must be positive and leave every link cell at least as wide as the range the grid was built for")

    def deform(self, scale):
        """set_box(box * scale); a scalar scales all three axes."""
        if self.host_only:
            raise RuntimeError("deform: a host-only simulation has no atoms to remap (set_box changes its geometry)")
        np = self._np
        self.set_box(self.box * np.broadcast_to(np.asarray(scale, dtype=np.float64), (3,)))

    def set_strain_rate(self, rates_per_ps):
        """Engineering strain rates (x, y, z) in 1/ps for the coming step() calls (1e9/s = 0.001; negative compresses): at the top of every step the box is
        set to box0 (1 + strain), the strain growing by rate dt / 1000 per step from its current value, and the positions are remapped with it.
        (0, 0, 0) switches it off.  A scalar is refused: say which axes."""
        if self.host_only:
            raise RuntimeError("set_strain_rate: a host-only simulation has no integrator")
        np = self._np
        r = np.asarray(rates_per_ps, dtype=np.float64)
        if r.shape != (3,):
            raise ValueError(f"set_strain_rate: need three rates (x, y, z) in 1/ps (got {rates_per_ps!r})")
        r = np.ascontiguousarray(r)
        if self.lib.comdSetStrainRate(self.ptr, r.ctypes.data_as(c_double_p)) != 0:
            raise ValueError(f"set_strain_rate: rates {r.tolist()} refused (not finite, the simulation runs in profile mode -s, or an axis is under the barostat)")

    # --- dynamics (not in the reference: comd-hip --msd, --msdStart, --msdFile) ---
    def track_displacement(self, on=True):
        """Start tracking every atom's unwrapped displacement from the current state (already tracking: the origin moves to the current state), or,
        with on=False, stop and free the device memory.  The drift kernels of the integrator add dt p/m of each atom they move into a 64-bit
        fixed-point record per global atom id (units of 2^-32 Angstroms), so periodic wraps, cell changes and migration between ranks do not show.
        Every rank of a multi-rank run makes the call.  RuntimeError when the device refuses the memory (32 bytes per global atom on every rank)."""
        if self.host_only:
            raise RuntimeError("track_displacement: a host-only simulation has no integrator")
        if self.lib.comdTrackDisplacement(self.ptr, 1 if on else 0) != 0:
            raise RuntimeError(f"track_displacement: no device memory for the displacement records of {self.n_global} atoms")
        self._tracking = bool(on)

    def _need_tracking(self, what):
        if not getattr(self, "_tracking", False):
            raise ValueError(f"{what}: displacements are not tracked (call track_displacement() first)")

    def displacements(self):
        """(n_global, 3) float64: the unwrapped displacement of every atom since track_displacement(), in Angstroms, keyed by gid: the ranks'
        integer records summed, the same array on every rank."""
        np = self._np
        self._need_tracking("displacements")
        out = np.zeros((self.n_global, 3), dtype=np.float64)
        rc = self.lib.comdDisplacements(self.ptr, out.ctypes.data_as(c_double_p))
        if rc != 0:
            raise RuntimeError(f"displacements: refused ({rc}): a component beyond 2^53 units of 2^-32 Angstroms")
        return out

    def msd(self, remove_drift=False):
        """(msd, (msd_x, msd_y, msd_z)) in Angstroms^2: the mean over all atoms of |d|^2 and of its three parts, d the displacement since
        track_displacement().  remove_drift: the mean displacement (the drift of the centre of mass, which a Langevin thermostat does not hold
        still) is taken out, msd_c = <d_c^2> - <d_c>^2.  One rank: reduced on the device; several: summed on the host from displacements()."""
        self._need_tracking("msd")
        out = (ctypes.c_double * 7)()
        rc = self.lib.comdMsd(self.ptr, out)
        if rc != 0:
            raise RuntimeError(f"msd: refused ({rc})")
        n = out[6]
        parts = tuple(out[3 + c] / n - ((out[c] / n) ** 2 if remove_drift else 0.0) for c in range(3))
        return parts[0] + parts[1] + parts[2], parts

    @property
    def n_global(self):
        return self.lib.comdNumGlobal(self.ptr)

    def gather(self, which, out=None):
        """Per-atom array of this rank's local atoms keyed by gid: 0 r, 1 p, 2 f -> (n,3); 3 e, 4 rhobar, 5 dfEmbed -> (n,)."""
        np = self._np
        n = self.n_global
        if out is None:
            out = np.zeros((n, 3) if which < 3 else (n,), dtype=np.float64)
        self.lib.comdGatherByGid(self.ptr, which, out.ctypes.data_as(c_double_p))
        return out

    def scatter(self, which, arr):
        np = self._np
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        self.lib.comdScatterByGid(self.ptr, which, arr.ctypes.data_as(c_double_p))

    def cells(self):
        """Slot arrays (device state copied to the host mirror; host mirror only when host_only):
        dict of nAtoms [nTotalBoxes], gid [nTotalBoxes, maxAtoms] and r/p/f components."""
        np = self._np
        h = (self.lib.comdHostAtoms if self.host_only else self.lib.comdFetchAtoms)(self.ptr).contents
        nb, cap = self.n_total_boxes, self.max_atoms
        out = {"nAtoms": np.ctypeslib.as_array(h.nAtoms, shape=(nb,)).copy(),
               "gid": np.ctypeslib.as_array(h.gid, shape=(nb, cap)).copy()}
        for k in ("rx", "ry", "rz", "px", "py", "pz", "fx", "fy", "fz", "e"):
            out[k] = np.ctypeslib.as_array(getattr(h, k), shape=(nb, cap)).copy()
        return out

    def box_from_tuple(self, ix, iy, iz):
        return self.lib.comdSimBoxFromTuple(self.ptr, ix, iy, iz)

    def box_from_coord(self, r):
        v = (ctypes.c_double * 3)(*r)
        return self.lib.comdSimBoxFromCoord(self.ptr, v)

    def face_cells(self, kind, face):
        np = self._np
        n = self.lib.comdFaceCells(self.ptr, kind, face, None)
        a = np.zeros(n, dtype=np.int32)
        self.lib.comdFaceCells(self.ptr, kind, face, a.ctypes.data)
        return a

    def neighbor_ranks(self):
        nbr = (ctypes.c_int * 6)()
        coord = (ctypes.c_int * 3)()
        self.lib.comdNeighborRanks(self.ptr, nbr, coord)
        return list(nbr), list(coord)

    def close(self):
        if self.ptr:
            self.lib.comdDestroy(self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def heat_flux_acf(j, window):
    """float64 (window, 3): the autocorrelation C_a(k) = (1 / (samples - k)) sum_t j[t, a] j[t + k, a] of a series j (samples, 3), 0 <= k < window <= samples
    (comdHeatFluxAcf of the host library; no device).  ValueError for another shape or window."""
    import numpy as np
    j = np.ascontiguousarray(j, dtype=np.float64)
    if j.ndim != 2 or j.shape[1] != 3 or not 1 <= int(window) <= j.shape[0]:
        raise ValueError(f"heat_flux_acf: need a series (samples, 3) and 1 <= window <= samples (got {j.shape}, {window})")
    out = np.zeros((int(window), 3), dtype=np.float64)
    if lib_host().comdHeatFluxAcf(j.ctypes.data_as(c_double_p), j.shape[0], int(window), out.ctypes.data_as(c_double_p)) != 0:
        raise ValueError("heat_flux_acf: comdHeatFluxAcf refused the series")
    return out


def _cubic_averages(c):
    return {"C11": float((c[0, 0] + c[1, 1] + c[2, 2]) / 3.0), "C12": float((c[0, 1] + c[0, 2] + c[1, 2]) / 3.0), "C44": float((c[3, 3] + c[4, 4] + c[5, 5]) / 3.0)}


def elastic_constants(born, stress, volume, temperature, n_atoms):
    """The stress-fluctuation elastic constants (Squire, Holt, Hoover 1969) of S samples of a fixed box (comdElasticConstants of the host library; no device):
        C_IJ = <B_IJ> / V - (V / kB T) (<s_I s_J> - <s_I> <s_J>) + (N kB T / V) kappa_IJ,  kappa = diag(2, 2, 2, 1, 1, 1)
    born (S, 6, 6) in eV (Simulation.born_matrix()), stress (S, 6) the pair stress -W / V in eV/A^3, volume in A^3, temperature in K.  With temperature = 0 or
    S = 1 only the Born part is there.  Returns {"C", "born", "fluctuation", "kinetic"} (6 x 6 each, eV/A^3; C is their sum), the cubic averages "C11", "C12",
    "C44" and "K" = (C11 + 2 C12) / 3, "G_V" = (C11 - C12 + 3 C44) / 5, "A" = 2 C44 / (C11 - C12), "cauchy_pressure" = C12 - C44.  These are derivatives with
    respect to the Lagrangian strain: under stress they differ from stress-strain coefficients by terms in the stress.  ValueError for mismatched shapes."""
    import numpy as np
    born = np.ascontiguousarray(born, dtype=np.float64)
    stress = np.ascontiguousarray(stress, dtype=np.float64)
    if born.ndim != 3 or born.shape[1:] != (6, 6) or stress.ndim != 2 or stress.shape[1] != 6 or born.shape[0] != stress.shape[0] or born.shape[0] < 1:
        raise ValueError(f"elastic_constants: need born (S, 6, 6) and stress (S, 6) with S >= 1 (got {born.shape}, {stress.shape})")
    if not (volume > 0.0 and temperature >= 0.0 and n_atoms >= 0):
        raise ValueError(f"elastic_constants: need volume > 0, temperature >= 0, n_atoms >= 0 (got {volume}, {temperature}, {n_atoms})")
    iu = np.triu_indices(6)
    tri = np.ascontiguousarray(born[:, iu[0], iu[1]] / float(volume))
    parts = [np.zeros((6, 6), dtype=np.float64) for _ in range(3)]
    if lib_host().comdElasticConstants(tri.ctypes.data_as(c_double_p), stress.ctypes.data_as(c_double_p), born.shape[0], float(volume), float(temperature),
                                       float(n_atoms), *[q.ctypes.data_as(c_double_p) for q in parts]) != 0:
        raise ValueError("elastic_constants: comdElasticConstants refused the samples")
    c = (parts[0] + parts[1]) + parts[2]
    out = {"C": c, "born": parts[0], "fluctuation": parts[1], "kinetic": parts[2]}
    out.update(_cubic_averages(c))
    c11, c12, c44 = out["C11"], out["C12"], out["C44"]
    out.update(K=(c11 + 2.0 * c12) / 3.0, G_V=(c11 - c12 + 3.0 * c44) / 5.0, A=2.0 * c44 / (c11 - c12) if c11 != c12 else float("nan"), cauchy_pressure=c12 - c44)
    return out


def berendsen_scale(p, target, dt_coupling, tau, modulus, axes="xyz", iso=False):
    """float64 (3,): the Berendsen scale factors mu_a = (1 - (dt_coupling / tau) (target_a - p_a) / modulus)^(1/3) on the axes of `axes`, 1 on the others;
    iso=True: one mu from the means over the chosen axes (comdBerendsenScale of the host library; no device).  p and target are scalars or (x, y, z), positive
    when compressive, in the unit of modulus.  ValueError for what the routine refuses: a non-finite argument, tau <= 0, modulus <= 0, dt_coupling > tau, no axis."""
    import numpy as np
    ax = str(axes)
    if len(set(ax)) != len(ax) or any(c not in "xyz" for c in ax):
        raise ValueError(f"berendsen_scale: axes must be a subset of 'xyz' (got {axes!r})")
    mask = sum(1 << "xyz".index(c) for c in ax)
    pp = np.ascontiguousarray(np.broadcast_to(np.asarray(p, dtype=np.float64), (3,)))
    tt = np.ascontiguousarray(np.broadcast_to(np.asarray(target, dtype=np.float64), (3,)))
    mu = np.ones(3, dtype=np.float64)
    if lib_host().comdBerendsenScale(pp.ctypes.data_as(c_double_p), tt.ctypes.data_as(c_double_p), float(dt_coupling), float(tau), float(modulus), mask,
                                     int(bool(iso)), mu.ctypes.data_as(c_double_p)) != 0:
        raise ValueError(f"berendsen_scale: refused (p {pp.tolist()}, target {tt.tolist()}, dt {dt_coupling}, tau {tau}, modulus {modulus}, axes {axes!r})")
    return mu


def muller_plathe_match(cold, hot, k):
    """(pairs int64 (n, 2), delta_e, skipped): comdMullerPlatheMatch of the host library (no device) on two candidate tables, float64 (rows, 6) each, a row
    {KE, gid + 1, p_x, p_y, p_z, slot} and a row of zeros empty -- the rows of all ranks one after the other.  The global top k of each table in list order (cold:
    KE descending, hot: KE ascending, the lower gid first among equal KE) are paired rank for rank and kept while KE_cold-slab > KE_hot-slab; from the first pair
    that fails on all are skipped.  pairs holds gids (cold-slab atom, hot-slab atom), delta_e = sum (KE_cold-slab - KE_hot-slab), skipped = k - n."""
    import numpy as np
    c = np.ascontiguousarray(cold, dtype=np.float64).reshape(-1, 6)
    h = np.ascontiguousarray(hot, dtype=np.float64).reshape(-1, 6)
    k = int(k)
    if not 1 <= k <= 64:
        raise ValueError(f"muller_plathe_match: k must lie in 1..64 (got {k})")
    rows = np.zeros((k, 2), dtype=np.int32)
    d_e = ctypes.c_double(0.0)
    kept = lib_host().comdMullerPlatheMatch(c.ctypes.data_as(c_double_p), c.shape[0], h.ctypes.data_as(c_double_p), h.shape[0], k, rows.ctypes.data_as(c_int_p),
                                            ctypes.byref(d_e))
    pairs = np.stack([c[rows[:kept, 0], 1] - 1.0, h[rows[:kept, 1], 1] - 1.0], axis=1).astype(np.int64).reshape(kept, 2)
    return pairs, d_e.value, k - kept


def fourier_conductivity(temperature, width, area, energy, time):
    """(gradient in K/A, kappa in W/(m K)) by Fourier's law from a Mueller-Plathe run (comdFourierKappa of the host library; no device): `temperature` the
    time-averaged slab temperatures of an even number of slabs `width` Angstroms wide, slab 0 cold and the middle slab hot; the two halves are folded (bin b with
    bin n - b) and a least-squares line goes through the folded interior bins; q = energy / (2 area time) with energy in eV, area in A^2, time in fs;
    kappa = q / gradient x 1.602176634e6.  kappa is None for a zero gradient or a non-positive area or time; both are None with fewer than two interior bins
    that have a temperature (NaN marks an empty slab)."""
    import numpy as np
    t = np.ascontiguousarray(temperature, dtype=np.float64).ravel()
    g, kappa = ctypes.c_double(0.0), ctypes.c_double(0.0)
    rc = lib_host().comdFourierKappa(t.ctypes.data_as(c_double_p), t.shape[0], float(width), float(area), float(energy), float(time), ctypes.byref(g), ctypes.byref(kappa))
    if rc < 0:
        return None, None
    return g.value, (kappa.value if rc == 0 else None)


_SK_WHY = {1: "k_max must lie in 1..64", 2: "every stride must be >= 1", 3: "stride * k_max must not exceed 65536"}


def _sk_grid(what, k_max, stride):
    """(k_max, int32 strides (3,)) after the refusals of comdStructureFactorRefusal, which come before any launch"""
    import numpy as np
    st = np.asarray(stride)
    if st.shape not in ((), (3,)) or not np.issubdtype(st.dtype, np.integer) or int(k_max) != k_max or np.any(np.abs(st) > 2 ** 30):
        raise ValueError(f"{what}: k_max is an int and stride an int or (sx, sy, sz) of ints (got {k_max!r}, {stride!r})")
    st = np.ascontiguousarray(np.broadcast_to(st, (3,)), dtype=np.int32)
    m = int(k_max) if abs(int(k_max)) < 2 ** 30 else 0      # beyond a C int: refused as 0 is
    why = lib_host().comdStructureFactorRefusal(m, st.ctypes.data_as(c_int_p))
    if why:
        raise ValueError(f"{what}: {_SK_WHY[why]} (got k_max {k_max}, stride {stride})")
    return m, st


def _sk_index(np, m):
    """int32 (K, 3): the (h, k, l) of the rows of the half grid in their C order"""
    h, k, l = np.meshgrid(np.arange(m + 1), np.arange(-m, m + 1), np.arange(-m, m + 1), indexing="ij")
    return np.stack([h.ravel(), k.ravel(), l.ravel()], axis=1).astype(np.int32)


def structure_factor_radial(rho, k_max, stride, box, n_bins):
    """(k centres, S, counts): the powder average of the density amplitudes `rho`, complex (K,) or any shape of K = (k_max + 1) (2 k_max + 1)^2 values in the C order of
    Simulation.structure_factor, on a box of extents `box` (comdStructureFactorRadial of the host library; no device).  S = |rho|^2 / N with N = Re rho(0, 0, 0).
    n_bins uniform |k| bins up to k_top = min_a 2 pi stride_a k_max / box_a: a vector with 0 < |k| <= k_top is in bin min(floor(|k| / (k_top / n_bins)), n_bins - 1)
    and counts twice when h > 0 (it stands for -k as well), once when h = 0; k = 0 is left out.  S is the weighted mean per bin, NaN where counts is 0.  ValueError
    for a refused grid, n_bins outside 1..4096, another number of amplitudes, a box extent or an N that is not positive."""
    import numpy as np
    m, st = _sk_grid("structure_factor_radial", k_max, stride)
    n = int(n_bins)
    amp = np.ascontiguousarray(rho, dtype=np.complex128).ravel()
    ext = np.ascontiguousarray(box, dtype=np.float64).ravel()
    if amp.shape[0] != (m + 1) * (2 * m + 1) ** 2 or ext.shape[0] != 3:
        raise ValueError(f"structure_factor_radial: need {(m + 1) * (2 * m + 1) ** 2} amplitudes and 3 box extents (got {amp.shape[0]}, {ext.shape[0]})")
    if not 1 <= n <= 4096:
        raise ValueError(f"structure_factor_radial: n_bins must lie in 1..4096 (got {n_bins})")
    raw = np.ascontiguousarray(np.stack([amp.real, amp.imag], axis=1))
    centres, s, counts = np.zeros(n), np.zeros(n), np.zeros(n)
    rc = lib_host().comdStructureFactorRadial(raw.ctypes.data_as(c_double_p), m, st.ctypes.data_as(c_int_p), ext.ctypes.data_as(c_double_p), n,
                                              centres.ctypes.data_as(c_double_p), s.ctypes.data_as(c_double_p), counts.ctypes.data_as(c_double_p))
    if rc != 0:
        raise ValueError(f"structure_factor_radial: refused ({rc}): the box extents and N = Re rho(0, 0, 0) = {amp[(m * (2 * m + 1) + m)].real} must be positive")
    return centres, s, counts.astype(np.int64)


def run_main(args):
    """The reference's main() (CoMD.c:86-187): full stdout report + YAML file."""
    argc, argv = _argv(list(args))
    return lib_host().comdMain(argc, argv)


class GlooTransport:
    """CommTransport backed by torch.distributed (gloo): host staging, any number of processes per GPU.

    The production transport is RCCL over xGMI (rccl_transport).  This one exists so that the multi-rank host logic
    can be exercised where RCCL cannot run: on CPU-only machines (host buffers, the CPU test-suite) and with several
    ranks sharing ONE GPU (device buffers are staged through pinned-less host copies).  It plays the role the
    reference's plain-MPI path does (haloExchange.c:1493-1522 + parallel.c:100-118).
    """

    def __init__(self, dist):
        import numpy as np
        import torch
        self.dist, self.torch, self.np = dist, torch, np
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.hip = None
        self.n_sized = 0          # exchanges that went through the pre-agreed-size path (tests look at it)
        self._keep = (SENDRECV_FN(self._guard(self._sendrecv)), SENDRECV2_FN(self._guard(self._sendrecv2)), ALLREDUCE_FN(self._guard(self._allreduce)),
                      BCAST_FN(self._guard(self._bcast)), BARRIER_FN(self._guard(self._barrier)), SENDRECV2SIZED_FN(self._guard(self._sendrecv2sized)))
        self.struct = CommTransport(None, *self._keep)

    @staticmethod
    def _guard(fn):
        """ctypes swallows exceptions raised inside callbacks (the C caller would carry on with garbage): make them fatal."""
        def wrapped(*args):
            try:
                return fn(*args)
            except BaseException:
                import traceback
                traceback.print_exc()
                sys.stderr.flush()
                os._exit(70)
        return wrapped

    def _exchange(self, send_bytes, dest, source, recv_cap):
        torch, dist = self.torch, self.dist
        n_send = torch.tensor([len(send_bytes)], dtype=torch.int64)
        n_recv = torch.zeros(1, dtype=torch.int64)
        if dest == self.rank and source == self.rank:
            return bytes(send_bytes)
        reqs = [dist.isend(n_send, dest, tag=1), dist.irecv(n_recv, source, tag=1)]
        for r in reqs:
            r.wait()
        n = int(n_recv[0])
        if n > recv_cap:
            raise RuntimeError(f"incoming message of {n} bytes exceeds the {recv_cap}-byte buffer")
        out = torch.empty(max(n, 1), dtype=torch.uint8)
        payload = torch.frombuffer(bytearray(send_bytes), dtype=torch.uint8) if len(send_bytes) else torch.zeros(1, dtype=torch.uint8)
        reqs = []
        if len(send_bytes):
            reqs.append(dist.isend(payload, dest, tag=2))
        if n:
            reqs.append(dist.irecv(out, source, tag=2))
        for r in reqs:
            r.wait()
        return out.numpy()[:n].tobytes()

    def _sendrecv(self, ctx, send_buf, send_len, dest, recv_buf, recv_cap, source, device, stream):
        if device:
            hip = self.hip or lib_hip()
            hip.comdStreamSynchronize(ctypes.c_void_p(stream))
            staging = ctypes.create_string_buffer(max(send_len, 1))
            if send_len:
                hip.comdMemcpyDtoH(staging, ctypes.c_void_p(send_buf), ctypes.c_long(send_len))
            data = self._exchange(staging.raw[:send_len], dest, source, recv_cap)
            if data:
                up = ctypes.create_string_buffer(data, len(data))
                hip.comdMemcpyHtoD(ctypes.c_void_p(recv_buf), up, ctypes.c_long(len(data)))
        else:
            data = self._exchange(ctypes.string_at(send_buf, send_len), dest, source, recv_cap)
            ctypes.memmove(recv_buf, data, len(data))
        return len(data)

    def _sendrecv2(self, ctx, send_m, n_m, dst_m, recv_p, send_p, n_p, dst_p, recv_m, recv_cap, device, stream, n_recv):
        # same pairing as the RCCL transport: my minus-face message lands in dst_m's "from plus" buffer and vice versa
        n_recv[0] = self._sendrecv(ctx, send_m, n_m, dst_m, recv_p, recv_cap, dst_p, device, stream)
        n_recv[1] = self._sendrecv(ctx, send_p, n_p, dst_p, recv_m, recv_cap, dst_m, device, stream)

    def _sendrecv2sized(self, ctx, send_m, n_m, dst_m, recv_p, n_rp, send_p, n_p, dst_p, recv_m, n_rm, device, stream):
        """Both ends agree on every size: payloads only, no size messages (the RCCL transport's rcclSendrecv2Sized)."""
        torch, dist = self.torch, self.dist
        if not device:
            raise RuntimeError("sized exchange is a device-buffer path")
        hip = self.hip or lib_hip()
        hip.comdStreamSynchronize(ctypes.c_void_p(stream))
        self.n_sized += 1

        def down(ptr, n):
            buf = ctypes.create_string_buffer(max(n, 1))
            if n:
                hip.comdMemcpyDtoH(buf, ctypes.c_void_p(ptr), ctypes.c_long(n))
            return torch.frombuffer(bytearray(buf.raw[:max(n, 1)]), dtype=torch.uint8)

        out_m, out_p = down(send_m, n_m), down(send_p, n_p)
        in_p, in_m = torch.empty(max(n_rp, 1), dtype=torch.uint8), torch.empty(max(n_rm, 1), dtype=torch.uint8)
        if dst_m == self.rank and dst_p == self.rank:          # loopback
            assert n_m == n_rp and n_p == n_rm
            in_p[:n_rp] = out_m[:n_m]
            in_m[:n_rm] = out_p[:n_p]
        else:
            # posting order as in RCCL: minus-face message first -- with dst_m == dst_p the peer's first send meets my first receive
            reqs = [dist.isend(out_m, dst_m, tag=3), dist.isend(out_p, dst_p, tag=4),
                    dist.irecv(in_p, dst_p, tag=3), dist.irecv(in_m, dst_m, tag=4)]
            for r in reqs:
                r.wait()
        for ptr, t, n in ((recv_p, in_p, n_rp), (recv_m, in_m, n_rm)):
            if n:
                raw = t.numpy()[:n].tobytes()
                hip.comdMemcpyHtoD(ctypes.c_void_p(ptr), ctypes.create_string_buffer(raw, n), ctypes.c_long(n))

    def _allreduce(self, ctx, buf, count, dtype):
        np, torch, dist = self.np, self.torch, self.dist
        ctype = ctypes.c_double if dtype == 1 else ctypes.c_float if dtype == 3 else ctypes.c_int
        arr = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctype)), shape=(count,))
        t = torch.from_numpy(arr.copy())
        if dtype in (1, 3) and self.world > 2:
            # floating-point sums in RANK ORDER (gather, then add 0, 1, 2, ...): the result does not depend on gloo's reduction tree, so
            # runs are reproducible and comparable bit for bit with a serial sum over the ranks (what the tests' checker does)
            parts = [torch.empty_like(t) for _ in range(self.world)]
            dist.all_gather(parts, t)
            acc = parts[0].clone()
            for p in parts[1:]:
                acc += p
            arr[:] = acc.numpy()
            return
        dist.all_reduce(t, op=dist.ReduceOp.MAX if dtype == 2 else dist.ReduceOp.SUM)
        arr[:] = t.numpy()

    def _bcast(self, ctx, buf, length, root):
        np, torch = self.np, self.torch
        arr = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)), shape=(length,))
        t = torch.from_numpy(arr.copy())
        self.dist.broadcast(t, src=root)
        arr[:] = t.numpy()

    def _barrier(self, ctx):
        self.dist.barrier()
