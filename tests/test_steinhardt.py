"""Steinhardt's bond-orientational order q4, q6, w4, w6 (computeSteinhardt, computeSteinhardtSummary, comdSteinhardt, comdSteinhardtSummary,
Simulation.steinhardt / steinhardt_summary / solid_like, comd-hip --steinhardt).

CoMD has no structural analysis, so nothing here is compared with a recorded number.  The reference is an O(N^2) minimum-image computation on the
gathered positions in float64 numpy, in blocks of 256 rows as test_csp's, with two independent routes:

    q_l^2   the addition theorem, q_l^2 = (1/144) sum_{a,b} P_l(u_a . u_b), with numpy.polynomial.legendre: no harmonic is formed;
    w_l     explicit Y_lm = N_lm P_l^m(cos theta) exp(i m phi) from the angles, P_l^m by differentiating numpy's Legendre series, all 2l + 1 components, the
            full triple sum over m1 + m2 + m3 = 0 with Wigner 3j symbols from the Racah formula in exact fractions (_wigner3j).  The same harmonics give
            q_l^2 a second time; the two routes agree to 1e-13 (a CPU test).

The only discrete decision is which neighbour is the 12th; test_csp's rule and caps:

    an atom whose 13th and 12th nearest distances differ by less than DELTA (`gap`), or whose count of neighbours inside the cutoff passes 12 within DELTA
    of the cutoff (`unsure`), is left out.

    build   DELTA      cap on the atoms left out (asserted before anything is compared)
    fp64    1e-9 A     0
    fp32    1e-4 A     0.5 %

Atoms whose reference q_l^2 is below 1e-3 are left out of the w_l comparison (w_l = W / S^(3/2) amplifies an error by 1 / q_l^2); cap 0, asserted with the
other masks.  The one exception is constructed: the centre of the icosahedron, whose q4 is 0 by symmetry (its test allows that one atom and says so).

Tolerances, on q_l^2 (not q_l: the square root amplifies an error at q = 0).  A unit vector inherits about two coordinate roundings over a shortest distance
of about 2.2 A, and |P_l'| <= l (l + 1) / 2:

    build   coordinate rounding (A)   derived bound on q4^2 / q6^2     allowed on q4^2 / q6^2
    fp64    7e-15                     <= 1.3e-13 / 2.7e-13             1e-11 / 1e-11
    fp32    3.8e-6                    <= 7e-5 / 1.5e-4                 1.5e-4 / 3e-4

and 6 tol(q_l^2) / q_l^2(ref) on w_l.  NaN masks compare exactly.
"""
import json
import math
import os
import re
import subprocess
import sys
import textwrap
from fractions import Fraction

import numpy as np
import pytest
from numpy.polynomial import legendre

import device_isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "comd-cuda-async_amd", "csrc")

SIGMA, LAT = 2.315, 3.615
MISHIN = ["-e", "-t", "setfl", "-p", "Cu01.eam.alloy"]
ADAMS = ["-e"]
RC = {"lj5": 5.0 * SIGMA, "lj2.5": 2.5 * SIGMA, "adams": 4.95, "mishin": 5.506786}
POT = {"lj5": [], "lj2.5": ["--ljCutoffSigmas", 2.5], "adams": ADAMS, "mishin": MISHIN}
DELTA64, DELTA32, CAP32 = 1e-9, 1e-4, 0.005
TOL64, TOL32 = (1e-11, 1e-11), (1.5e-4, 3e-4)                    # on q4^2, q6^2
SMALL = 1e-3                                                     # reference q_l^2 below this: no w_l comparison
SPARSE = ["-e", "-x", 4, "-y", 5, "-z", 6, "-l", 7.0, "-r", 0.5]          # test_csp's: 2 to 10 neighbours, empty cells
LJ_METHODS = [("thread_atom", []), ("warp_atom", []), ("cta_cell", []), ("cta_cell", ["-L", "-S", 0.03]), ("thread_atom_nl", []),
              ("thread_atom", ["-H"]), ("thread_atom", ["-a", 1]), ("cta_cell", ["-a", 1])]
EAM_METHODS = [("thread_atom", []), ("warp_atom", []), ("cta_cell", []), ("thread_atom_nl", []), ("cta_cell", ["-H"]), ("cta_cell", ["-a", 1]),
               ("thread_atom", ["-a", 1])]                       # test_csp's lists
ICO_ARGS = ["-e", "-x", 4, "-y", 5, "-z", 6, "-l", 7.2]
ICO_EXTENT = (4 * 7.2, 5 * 7.2, 6 * 7.2)
ICO_CENTRE = np.array([17.3, 20.6, 21.65])                      # test_cna's: near a corner of the link cells, the 13 atoms spread over 8 cells
# 12 ideal neighbours: q4, q6, w4, w6 (None: 0/0)
IDEAL = {"fcc": (0.190940654, 0.574524260, -0.159317373, -0.013160601), "hcp": (0.097222222, 0.484761685, 0.134097047, -0.012441959),
         "ico": (0.0, 0.663324958, None, -0.169753895)}


def _cube(n):
    return ["-x", n, "-y", n, "-z", n, "-l", repr(LAT)]


PRELUDE = f"import sys, json\nsys.path.insert(0, {ROOT!r})\nimport __graft_entry__ as ge\npkg = ge.load_package()\n"


def _child(code, env=None, timeout=600):
    return subprocess.run([sys.executable, "-c", PRELUDE + textwrap.dedent(code)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


# ---------------------------------------------------------------- numpy restatement
def _wigner3j(j1, j2, j3, m1, m2, m3):
    """The Racah formula, the sum and the argument of the root in exact fractions:
    (-1)^(j1 - j2 - m3) sqrt(Delta) sqrt(prod (j_i + m_i)! (j_i - m_i)!) sum_t (-1)^t / (t! (j3 - j2 + t + m1)! (j3 - j1 + t - m2)! (j1 + j2 - j3 - t)!
    (j1 - t - m1)! (j2 - t + m2)!),  Delta = (j1 + j2 - j3)! (j1 - j2 + j3)! (-j1 + j2 + j3)! / (j1 + j2 + j3 + 1)!"""
    f = math.factorial
    if m1 + m2 + m3 != 0 or abs(m1) > j1 or abs(m2) > j2 or abs(m3) > j3 or not abs(j1 - j2) <= j3 <= j1 + j2:
        return 0.0
    total = Fraction(0)
    for t in range(0, j1 + j2 - j3 + 1):
        args = (t, j3 - j2 + t + m1, j3 - j1 + t - m2, j1 + j2 - j3 - t, j1 - t - m1, j2 - t + m2)
        if min(args) < 0:
            continue
        den = 1
        for a in args:
            den *= f(a)
        total += Fraction((-1) ** t, den)
    delta = Fraction(f(j1 + j2 - j3) * f(j1 - j2 + j3) * f(-j1 + j2 + j3), f(j1 + j2 + j3 + 1))
    under = delta * f(j1 + m1) * f(j1 - m1) * f(j2 + m2) * f(j2 - m2) * f(j3 + m3) * f(j3 - m3)
    sign = -1.0 if (j1 - j2 - m3) % 2 else 1.0
    return sign * math.sqrt(under.numerator / under.denominator) * (total.numerator / total.denominator)


_W3J = {l: {(m1, m2): _wigner3j(l, l, l, m1, m2, -m1 - m2) for m1 in range(-l, l + 1) for m2 in range(-l, l + 1) if abs(m1 + m2) <= l} for l in (4, 6)}


def _harmonic_sums(u, l):
    """q_lm = mean over the 12 of Y_lm(u), all m = -l..l: complex (rows, 2l + 1), column l + m.  u: (rows, 12, 3) unit vectors"""
    c = np.clip(u[..., 2], -1.0, 1.0)
    s = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    phi = np.arctan2(u[..., 1], u[..., 0])
    q = np.zeros((u.shape[0], 2 * l + 1), dtype=np.complex128)
    for m in range(0, l + 1):
        plm = (-1.0) ** m * s ** m * legendre.Legendre.basis(l).deriv(m)(c) if m else legendre.Legendre.basis(l)(c)
        norm = math.sqrt((2 * l + 1) / (4.0 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
        y = norm * plm * np.exp(1j * m * phi)
        q[:, l + m] = y.mean(1)
        if m:
            q[:, l - m] = (-1.0) ** m * np.conj(q[:, l + m])
    return q


def _invariants(u):
    """(q2_add (rows, 2), q2_lm (rows, 2), w (rows, 2)) for l = 4, 6 of the sets u (rows, 12, 3) of unit vectors: q_l^2 by the addition theorem, q_l^2 and
    w_l from the explicit harmonics.  w_l is 0 where q_l^2 < 1e-6, as the kernel reports it."""
    cosines = np.clip(np.einsum("rak,rbk->rab", u, u), -1.0, 1.0)
    q2_add, q2_lm, w = np.zeros((len(u), 2)), np.zeros((len(u), 2)), np.zeros((len(u), 2))
    for col, l in enumerate((4, 6)):
        q2_add[:, col] = legendre.legval(cosines, [0.0] * l + [1.0]).sum((1, 2)) / 144.0
        q = _harmonic_sums(u, l)
        norm2 = (q.real ** 2 + q.imag ** 2).sum(1)
        q2_lm[:, col] = 4.0 * math.pi / (2 * l + 1) * norm2
        triple = np.zeros(len(u), dtype=np.complex128)
        for (m1, m2), t in _W3J[l].items():
            triple += t * q[:, l + m1] * q[:, l + m2] * q[:, l - m1 - m2]
        assert np.all(np.abs(triple.imag) <= 1e-12 * (1.0 + np.abs(triple.real)))
        with np.errstate(invalid="ignore", divide="ignore"):
            w[:, col] = np.where(q2_lm[:, col] < 1e-6, 0.0, triple.real / norm2 ** 1.5)
    return q2_add, q2_lm, w


def _numpy_steinhardt(pos, extent, rc, delta):
    """dict of per-atom q2 (n, 2) by the addition theorem, q2_lm (n, 2) and w (n, 2) from the harmonics, valid (12 neighbours inside the cutoff), gap (13th -
    12th nearest distance) and unsure (the count inside the cutoff passes 12 within delta of the cutoff), in blocks of 256 rows as test_csp._numpy_csp"""
    n = len(pos)
    extent = np.broadcast_to(np.asarray(extent, dtype=np.float64), (3,))
    q2, q2_lm, w = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    valid, gap, unsure = np.zeros(n, dtype=bool), np.full(n, np.inf), np.zeros(n, dtype=bool)
    for s in range(0, n, 256):
        d = pos[None, :, :] - pos[s:s + 256, None, :]                # R = r_j - r_i
        d -= np.rint(d / extent) * extent
        r2 = (d * d).sum(-1)
        rows = np.arange(len(r2))
        r2[rows, s + rows] = np.inf                                   # j != i
        r = np.sqrt(r2)
        near = np.argpartition(r2, 13, axis=1)[:, :14]
        near = np.take_along_axis(near, np.argsort(np.take_along_axis(r2, near, axis=1), axis=1), axis=1)[:, :13]
        r13 = np.take_along_axis(r, near, axis=1)
        gap[s:s + 256] = r13[:, 12] - r13[:, 11]
        valid[s:s + 256] = (r < rc).sum(1) >= 12
        unsure[s:s + 256] = ((r < rc + delta).sum(1) >= 12) != ((r < rc - delta).sum(1) >= 12)
        vec = np.take_along_axis(d, near[:, :12, None], axis=1)       # (rows, 12, 3)
        u = vec / r13[:, :12, None]
        q2[s:s + 256], q2_lm[s:s + 256], w[s:s + 256] = _invariants(u)
    out = {"q2": q2, "q2_lm": q2_lm, "w": w, "valid": valid, "gap": gap, "unsure": unsure}
    for a in out.values():
        a.setflags(write=False)
    return out


_REF = {}


def _reference(key, pos, extent, rc, delta):
    """computed once per key, never modified"""
    if key is None:
        return _numpy_steinhardt(pos, extent, rc, delta)
    if key not in _REF:
        _REF[key] = _numpy_steinhardt(pos, extent, rc, delta)
    return _REF[key]


def _left_out(ref, delta, single, small_cap=0):
    """(the atoms outside every comparison, the valid atoms outside the w4 / w6 comparison (n, 2)), after the caps of the module docstring"""
    n = len(ref["valid"])
    no = (ref["gap"] < delta) | ref["unsure"]
    small = ref["valid"][:, None] & (ref["q2"] < SMALL)
    assert no.sum() <= (CAP32 * n if single else 0), (int(no.sum()), n)
    assert small.sum() <= small_cap, (np.nonzero(small.any(1))[0].tolist(), ref["q2"][small.any(1)].tolist())
    return no, small


def _check(got, ref, single=False, what="", small_cap=0):
    """got: (n, 4) q4 q6 w4 w6 of the device against the reference, under the rules of the module docstring"""
    assert got.dtype == np.float64 and got.shape == (len(ref["valid"]), 4)
    no, small = _left_out(ref, DELTA32 if single else DELTA64, single, small_cap)
    keep = ~no
    tol = TOL32 if single else TOL64
    assert np.array_equal(np.isnan(got[keep]), np.repeat(~ref["valid"][keep, None], 4, axis=1)), what
    v = keep & ref["valid"]
    worst = []
    for col in (0, 1):
        dq = np.abs(got[v, col] ** 2 - ref["q2"][v, col]) if v.any() else np.zeros(1)
        vw = v & ~small[:, col]
        dw = np.abs(got[vw, 2 + col] - ref["w"][vw, col]) if vw.any() else np.zeros(1)
        allow = 6.0 * tol[col] / ref["q2"][vw, col] if vw.any() else np.ones(1)
        worst += [dq.max(), dw.max(), (dw / allow).max()]
    print(f"{what}: atoms {len(got)}, left out {int(no.sum())}, invalid {int((~ref['valid']).sum())}, small q4^2 / q6^2 {int(small[:, 0].sum())} / {int(small[:, 1].sum())}, "
          f"largest |difference| q4^2 {worst[0]:.3e} q6^2 {worst[3]:.3e} w4 {worst[1]:.3e} ({worst[2]:.3e} of its allowance) w6 {worst[4]:.3e} ({worst[5]:.3e})")
    assert worst[0] <= tol[0] and worst[3] <= tol[1], (what, worst)
    assert worst[2] <= 1.0 and worst[5] <= 1.0, (what, worst)
    if v.any():
        assert np.all(got[v, :2] >= 0.0) and np.all(got[v, :2] <= 1.0 + 1e-6)


def _against_numpy(sim, extent, rc, key=None, single=False, small_cap=0):
    pos = sim.gather(0)
    got = sim.steinhardt()
    assert abs(sim.cutoff - rc) <= 1e-6
    ref = _reference(key, pos, extent, sim.cutoff, DELTA32 if single else DELTA64)
    _check(got, ref, single, str(key), small_cap)
    return got


def _host_positions(pkg, args):
    """positions by gid of the initial state, from a host-only simulation (no device)"""
    with pkg.Simulation(args, host_only=True) as sim:
        c, ng = sim.cells(), sim.n_global
    pos = np.zeros((ng, 3))
    for b in range(sim.n_local_boxes):
        for o in range(c["nAtoms"][b]):
            pos[c["gid"][b, o]] = (c["rx"][b, o], c["ry"][b, o], c["rz"][b, o])
    return pos


_STATES = {}


def _stacking_fault(pkg, n=8):
    """test_cna's: (positions, gids that must be HCP, gids that must be FCC): every atom above a plane halfway between two (111) planes in mid-box is shifted
    by lat/6 (1, 1, -2), wrapped, +-0.05 A of noise.  The two sets: sites more than 1.5 lat from every box face, within 0.75 lat / sqrt 3 of the plane or not."""
    if ("fault", n) not in _STATES:
        sites = _host_positions(pkg, _cube(n) + ADAMS)
        height = sites.sum(1) / np.sqrt(3.0)
        plane = (1.5 * n + 0.25) * LAT / np.sqrt(3.0)
        pos = sites + np.where(height > plane, 1.0, 0.0)[:, None] * (LAT / 6.0) * np.array([1.0, 1.0, -2.0])
        pos += np.random.default_rng(20120521).uniform(-0.05, 0.05, pos.shape)
        pos = np.mod(pos, n * LAT)
        inner = np.all((sites > 1.5 * LAT) & (sites < (n - 1.5) * LAT), axis=1)
        close = np.abs(height - plane) < 0.75 * LAT / np.sqrt(3.0)
        pos.setflags(write=False)
        _STATES[("fault", n)] = (pos, np.nonzero(inner & close)[0], np.nonzero(inner & ~close)[0])
    return _STATES[("fault", n)]


def _ico_vertices():
    phi = 0.5 * (1.0 + np.sqrt(5.0))
    verts = np.array([p for a in (-1.0, 1.0) for b in (-phi, phi) for p in ((0.0, a, b), (a, b, 0.0), (b, 0.0, a))])
    return verts / np.sqrt(1.0 + phi * phi)


def _icosahedron(pkg):
    """test_cna's: (positions, gid of the centre, gids of the 12 vertices): the sparse lattice (no atom has a neighbour inside the cutoff) with +-0.02 A of
    noise, the 13 atoms nearest ICO_CENTRE moved onto a centre and the 12 vertices of an icosahedron of radius 2.5 A"""
    if "ico" not in _STATES:
        pos = _host_positions(pkg, ICO_ARGS)
        rng = np.random.default_rng(2012)
        order = np.argsort(((pos - ICO_CENTRE) ** 2).sum(1))[:13]
        pos[order[0]] = ICO_CENTRE
        pos[order[1:]] = ICO_CENTRE + 2.5 * _ico_vertices()
        pos += rng.uniform(-0.02, 0.02, pos.shape)
        pos.setflags(write=False)
        _STATES["ico"] = (pos, int(order[0]), np.sort(order[1:]))
    return _STATES["ico"]


def _apply(sim, pos):
    sim.scatter(0, pos)
    sim.redistribute()
    sim.compute_force()
    assert np.array_equal(sim.gather(0), pos)


def _ideal(name):
    """(1, 12, 3): the 12 unit vectors to the neighbours of an ideal FCC, HCP or icosahedral site"""
    if name == "fcc":
        v = [p for a in (-1.0, 1.0) for b in (-1.0, 1.0) for p in ((a, b, 0.0), (a, 0.0, b), (0.0, a, b))]
    elif name == "hcp":
        v = [(math.cos(k * math.pi / 3.0), math.sin(k * math.pi / 3.0), 0.0) for k in range(6)]
        for z in (-1.0, 1.0):
            v += [(math.cos(math.pi / 6.0 + 2.0 * k * math.pi / 3.0) / math.sqrt(3.0), math.sin(math.pi / 6.0 + 2.0 * k * math.pi / 3.0) / math.sqrt(3.0),
                   z * math.sqrt(2.0 / 3.0)) for k in range(3)]
    else:
        v = _ico_vertices()
    v = np.array(v, dtype=np.float64)
    assert v.shape == (12, 3)
    return (v / np.sqrt((v * v).sum(1))[:, None])[None]


_FCC_EXACT = {}


def _fcc_exact():
    """q4^2, q6^2, w4, w6 of the ideal FCC site from the numpy helper (the table of IDEAL has 9 digits, the fp64 tolerances ask for more)"""
    if not _FCC_EXACT:
        q2, _, w = _invariants(_ideal("fcc"))
        _FCC_EXACT["v"] = (q2[0, 0], q2[0, 1], w[0, 0], w[0, 1])
    return _FCC_EXACT["v"]


# ---------------------------------------------------------------- CPU: flags, exports, ISA, the reference itself
def test_steinhardt_flags_are_listed_and_accepted_host_only(pkg):
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--steinhardt', '--stSolid', 0.45, '--stFile', 'x.dat', '--stDump', 'd.xyz', '--stDumpMax', 0.3], "
                  "host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in ("steinhardt", "stSolid", "stFile", "stDump", "stDumpMax"):
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_steinhardt_is_exported_and_declared(sfx):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"libcomd_hip{sfx}.so")], capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "computeSteinhardt" in names and "computeSteinhardtSummary" in names
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"libcomd_host{sfx}.so")], capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "comdSteinhardt" in names and "comdSteinhardtSummary" in names
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void computeSteinhardt\(SimGpu\* sim, real_t\* outBySlot4\);", header, flags=re.M)
    assert re.search(r"^void computeSteinhardtSummary\(SimGpu\* sim, double threshold, double\* out\);", header, flags=re.M)


@pytest.mark.parametrize("precision", ["double", "single"])
def test_steinhardt_kernels_use_no_scratch(precision):
    """... and Steinhardt_thread_atom keeps the registers of its 4 waves per SIMD"""
    blocks = device_isa.blocks(precision, r"Steinhardt\w+")
    assert len(blocks) == 3 and any("Steinhardt_thread_atom" in n for n in blocks), sorted(blocks)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
    device_isa.assert_keeps_waves(blocks, "Steinhardt_thread_atom", 4)


def test_host_only_simulation_refuses(pkg):
    with pkg.Simulation(_cube(6) + ADAMS, host_only=True) as sim:
        for call in (sim.steinhardt, sim.steinhardt_summary, sim.solid_like):
            with pytest.raises(RuntimeError):
                call()


def test_wigner3j_helper():
    """closed forms: (4 4 4; 0 0 0)^2 = 18/1001, (6 6 6; 0 0 0)^2 = 400/46189 (negative), (2 2 2; 0 0 0) = -sqrt(2/35), (1 1 0; 1 -1 0) = 1/sqrt 3; the
    symmetries under permutation and sign change; orthogonality sum_{m1 m2} (2 j3 + 1) (j1 j2 j3; m1 m2 m3)^2 = 1"""
    assert abs(_wigner3j(4, 4, 4, 0, 0, 0) - math.sqrt(18.0 / 1001.0)) <= 1e-15
    assert abs(_wigner3j(6, 6, 6, 0, 0, 0) + math.sqrt(400.0 / 46189.0)) <= 1e-15
    assert abs(_wigner3j(2, 2, 2, 0, 0, 0) + math.sqrt(2.0 / 35.0)) <= 1e-15
    assert abs(_wigner3j(1, 1, 0, 1, -1, 0) - 1.0 / math.sqrt(3.0)) <= 1e-15
    for l in (4, 6):
        for (m1, m2), t in _W3J[l].items():
            m3 = -m1 - m2
            assert abs(t - _W3J[l][(m2, m1)]) <= 1e-15 and abs(t - _W3J[l][(m2, m3)]) <= 1e-15 and abs(t - _W3J[l][(-m1, -m2)]) <= 1e-15
        for m3 in range(-l, l + 1):
            total = sum((2 * l + 1) * t * t for (m1, m2), t in _W3J[l].items() if -m1 - m2 == m3)
            assert abs(total - 1.0) <= 1e-13, (l, m3, total)


@pytest.mark.parametrize("name", ["fcc", "hcp", "ico"])
def test_ideal_neighbour_sets(name):
    """the numpy helper reproduces the values of 12 ideal neighbours to 1e-8, by both routes, and under a rotation"""
    u = _ideal(name)
    rot = np.linalg.qr(np.random.default_rng(7).normal(size=(3, 3)))[0]
    for v in (u, u @ rot.T):
        q2_add, q2_lm, w = _invariants(v)
        q4, q6, w4, w6 = IDEAL[name]
        print(name, np.sqrt(np.maximum(q2_add[0], 0.0)).tolist(), w[0].tolist())
        assert np.all(np.abs(q2_add - q2_lm) <= 1e-13)
        assert abs(math.sqrt(max(q2_add[0, 0], 0.0)) - q4) <= 1e-8 and abs(math.sqrt(q2_add[0, 1]) - q6) <= 1e-8
        assert abs(w[0, 1] - w6) <= 1e-8
        if w4 is None:
            assert q2_lm[0, 0] <= 1e-20 and w[0, 0] == 0.0
        else:
            assert abs(w[0, 0] - w4) <= 1e-8


@pytest.mark.parametrize("pot,n", [("lj5", 8), ("lj2.5", 8), ("adams", 6), ("mishin", 6)])
def test_noisy_lattice_keeps_the_reference_inside_the_fp64_caps(pkg, pot, n):
    """The -r 0.1 states of the GPU tests, in numpy alone: no atom within DELTA64 of a tie, none with q_l^2 < 1e-3, and the two routes to q_l^2 agree to 1e-13"""
    pos = _host_positions(pkg, _cube(n) + ["-r", 0.1] + POT[pot])
    ref = _reference(("host", pot, n), pos, n * LAT, RC[pot], DELTA64)
    _left_out(ref, DELTA64, False)
    diff = np.abs(ref["q2"] - ref["q2_lm"]).max()
    q6 = np.sqrt(ref["q2"][:, 1])
    print(f"{pot} {n}: two routes differ by {diff:.3e}; q6 mean {q6.mean():.4f} min {q6.min():.4f} max {q6.max():.4f}; least q4^2 {ref['q2'][:, 0].min():.3e}")
    assert ref["valid"].all() and diff <= 1e-13
    assert 0.5 < q6.mean() < 0.5745 and np.all(ref["w"][:, 0] < 0.0)          # +-0.1 A of uniform noise: still an FCC crystal (mean q6 0.564)


def test_constructed_states_in_numpy(pkg):
    """the stacking fault and the icosahedron of the GPU tests: what they assert of the device holds for the reference"""
    pos, hcp, fcc = _stacking_fault(pkg)
    ref = _reference("fault", pos, 8 * LAT, RC["adams"], DELTA64)
    _left_out(ref, DELTA64, False)
    assert len(hcp) > 100 and len(fcc) > 300 and np.all(ref["w"][hcp, 0] > 0.0) and np.all(ref["w"][fcc, 0] < 0.0)
    pos, centre, verts = _icosahedron(pkg)
    ref = _reference("ico", pos, ICO_EXTENT, RC["adams"], DELTA64)
    no, small = _left_out(ref, DELTA64, False, small_cap=1)
    inside = set(np.nonzero(ref["valid"])[0].tolist())
    print("icosahedron: atoms with 12 neighbours inside the cutoff", sorted(inside), "centre", centre, "vertices", verts.tolist())
    assert centre in inside and inside <= {centre} | set(verts.tolist()) and small[centre, 0] and not small[centre, 1]
    assert abs(math.sqrt(ref["q2"][centre, 1]) - 0.6633) <= 0.01 and abs(ref["w"][centre, 1] + 0.1698) <= 0.01


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("pot,n,method", [("lj5", 8, "thread_atom"), ("lj2.5", 8, "thread_atom"), ("adams", 6, "thread_atom"),
                                          ("mishin", 6, "thread_atom"), ("lj5", 8, "cta_cell"), ("adams", 6, "cta_cell")])
def test_matches_numpy(gpu, pot, n, method):
    """Step 0 and after 10 steps.  lj5: cells of several 64-slot chunks, 2 cells per axis; lj2.5 and EAM: the replicated small-chunk path."""
    with gpu.Simulation(_cube(n) + ["-r", 0.1, "-m", method] + POT[pot]) as sim:
        assert abs(sim.cutoff - RC[pot]) <= 1e-6
        _against_numpy(sim, n * LAT, RC[pot], key=(pot, n, 0))          # step 0: the state does not depend on the method
        sim.step(10)
        _against_numpy(sim, n * LAT, RC[pot])


@pytest.mark.gpu
def test_perfect_fcc_lattice(gpu):
    """all 12 distances tie: whichever order the 12 come in, the FCC values"""
    q42, q62, w4, w6 = _fcc_exact()
    with gpu.Simulation(_cube(6) + ADAMS) as sim:
        got = sim.steinhardt()
        summary = sim.steinhardt_summary()
        solid = sim.solid_like()
    assert got.shape == (864, 4) and not np.isnan(got).any()
    print("perfect FCC: largest |difference|", np.abs(got[:, 0] ** 2 - q42).max(), np.abs(got[:, 1] ** 2 - q62).max(), np.abs(got[:, 2] - w4).max(), np.abs(got[:, 3] - w6).max())
    assert np.all(np.abs(got[:, 0] ** 2 - q42) <= TOL64[0]) and np.all(np.abs(got[:, 1] ** 2 - q62) <= TOL64[1])
    assert np.all(np.abs(got[:, 2] - w4) <= 6.0 * TOL64[0] / q42) and np.all(np.abs(got[:, 3] - w6) <= 6.0 * TOL64[1] / q62)
    assert summary["n"] == 864 and summary["invalid"] == 0 and summary["solid"] == 864 and abs(summary["mean_q6"] - math.sqrt(q62)) <= TOL64[1]
    assert np.array_equal(solid, np.arange(864, dtype=np.int64)) and solid.dtype == np.int64


@pytest.mark.gpu
def test_stacking_fault(gpu):
    pos, hcp, fcc = _stacking_fault(gpu)
    with gpu.Simulation(_cube(8) + ADAMS) as sim:
        _apply(sim, pos)
        got = _against_numpy(sim, 8 * LAT, RC["adams"], key="fault")
    print(f"stacking fault: {len(hcp)} HCP and {len(fcc)} FCC sites inside; w4 on them {got[hcp, 2].min():.4f} .. {got[hcp, 2].max():.4f} and "
          f"{got[fcc, 2].min():.4f} .. {got[fcc, 2].max():.4f}")
    assert len(hcp) > 100 and len(fcc) > 300
    assert np.all(got[hcp, 2] > 0.0) and np.all(got[fcc, 2] < 0.0)


@pytest.mark.gpu
def test_icosahedron(gpu):
    """The centre's q4 is 0 by symmetry (here 1e-3 and less, from the +-0.02 A of noise): it is the one atom the rule on small q_l^2 may leave out of the w4
    comparison.  Every atom of the sparse lattice is invalid.  A vertex has the centre and 10 vertices inside the cutoff (the antipode, at 5 A, is not), and
    six of the twelve have a lattice atom inside it as well: those are valid in the numpy reference, and the NaN mask is compared with it exactly."""
    pos, centre, verts = _icosahedron(gpu)
    with gpu.Simulation(ICO_ARGS) as sim:
        _apply(sim, pos)
        got = _against_numpy(sim, ICO_EXTENT, RC["adams"], key="ico", small_cap=1)
        summary = sim.steinhardt_summary()
    print("icosahedron centre:", got[centre].tolist())
    assert abs(got[centre, 1] - 0.6633) <= 0.01 and abs(got[centre, 3] + 0.1698) <= 0.01 and got[centre, 0] ** 2 < SMALL
    rest = np.ones(len(got), dtype=bool)
    rest[centre] = False
    rest[verts] = False
    valid = ~np.isnan(got[:, 1])
    assert np.isnan(got[rest]).all() and not np.isnan(got[centre]).any() and np.array_equal(valid, _REF["ico"]["valid"])
    assert summary["n"] == valid.sum() and summary["invalid"] == 480 - valid.sum() and summary["max_q6"] == got[centre, 1]
    assert summary["min_q6"] == got[valid, 1].min() and summary["min_q6_gid"] == int(np.nonzero(valid)[0][np.argmin(got[valid, 1])])


@pytest.mark.gpu
def test_fewer_than_twelve_neighbours(gpu):
    with gpu.Simulation(SPARSE) as sim:
        got = _against_numpy(sim, (28.0, 35.0, 42.0), RC["adams"])
        summary = sim.steinhardt_summary()
        solid = sim.solid_like()
    assert got.shape == (480, 4) and np.isnan(got).all() and solid.size == 0
    assert summary == {"n": 0, "invalid": 480, "mean_q4": 0.0, "mean_q6": 0.0, "min_q6": 0.0, "min_q6_gid": -1, "max_q6": 0.0, "mean_w4": 0.0, "mean_w6": 0.0,
                       "solid": 0}, summary


@pytest.mark.gpu
@pytest.mark.parametrize("method,extra", [("thread_atom_nl", ["-S", 0.1]), ("cta_cell", ["-L", "-S", 0.03])])
def test_cells_that_are_not_rebinned(gpu, method, extra):
    """Between list builds the atoms keep their cells (sized cutoff + skin): the 27-cell walk still sees every neighbour within the cutoff."""
    n = 12
    with gpu.Simulation(_cube(n) + ["-T", 3000, "-m", method] + extra) as sim:
        sim.step(20)
        _against_numpy(sim, n * LAT, RC["lj5"])


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj5", 12), ("mishin", 10)])
def test_methods_and_layouts_agree(gpu, pot, n):
    """Step 0, the same state and halo images under every method, cell size, cell numbering and stream mode.  The 13 nearest distances of every atom are
    distinct, which fixes the 12 and the order of the sums: the same bits."""
    got = {}
    for method, extra in LJ_METHODS if pot.startswith("lj") else EAM_METHODS:
        with gpu.Simulation(_cube(n) + ["-r", 0.1, "-m", method] + extra + POT[pot]) as sim:
            got[" ".join([method] + [str(x) for x in extra])] = sim.steinhardt()
    first = got["thread_atom"]
    assert np.isfinite(first).all() and first[:, 1].min() > 0.0
    for name, q in got.items():
        print(pot, name, "largest |difference| to thread_atom", np.abs(q - first).max())
        assert np.array_equal(q, first), name


@pytest.mark.gpu
def test_arguments(gpu):
    n = 8
    with gpu.Simulation(_cube(n) + ["-r", 0.1]) as sim:
        cells = sim.cells()
        before = sim.steinhardt()
        for threshold in (0.0, 1.0, -1.0, 2.0):
            with pytest.raises(ValueError):
                sim.steinhardt_summary(threshold)
            with pytest.raises(ValueError):
                sim.solid_like(threshold)
        assert _same_cells(cells, sim.cells()) and np.array_equal(before, sim.steinhardt())
        q6 = before[:, 1]
        t = float(np.median(q6))
        solid = sim.solid_like(t)
        assert solid.dtype == np.int64 and np.array_equal(solid, np.nonzero(q6 >= t)[0]) and 0 < solid.size < len(q6)
        assert np.array_equal(sim.solid_like(), np.nonzero(q6 >= sim.STEINHARDT_SOLID)[0])
        summary = sim.steinhardt_summary(t)
        assert summary["solid"] == solid.size and summary["n"] == len(q6) and summary["invalid"] == 0
        assert summary["min_q6"] == q6.min() and summary["max_q6"] == q6.max() and summary["min_q6_gid"] == int(np.argmin(q6))
        for key, col in (("mean_q4", 0), ("mean_q6", 1), ("mean_w4", 2), ("mean_w6", 3)):
            assert abs(summary[key] - before[:, col].mean()) <= 1e-12, key


def _same_cells(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and set(a) == set(b)


@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj5", "adams"])
def test_purity_and_reproducibility(gpu, pot):
    args = _cube(8) + ["-r", 0.1] + POT[pot]
    with gpu.Simulation(args) as sim:
        cells, energy = sim.cells(), sim.energy()
        a = sim.steinhardt()
        s = sim.steinhardt_summary()
        b = sim.steinhardt()
        assert np.array_equal(a, b) and s == sim.steinhardt_summary()
        assert _same_cells(cells, sim.cells()) and energy == sim.energy()
        for _ in range(5):
            sim.step(1)
            sim.steinhardt()
            sim.steinhardt_summary()
        with_calls = (sim.cells(), sim.energy())
    with gpu.Simulation(args) as sim:
        for _ in range(5):
            sim.step(1)
        assert _same_cells(with_calls[0], sim.cells()) and with_calls[1] == sim.energy()


def _ranks(tmp_path, grid, args, timeout=900):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    assert world <= 8
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "steinhardt_worker.py"), str(r), str(world), port, *map(str, grid), str(tmp_path), json.dumps(args)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=timeout)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "Steinhardt saved" in out, f"rank {r} failed:\n{out[-3000:]}"
    return [np.load(os.path.join(str(tmp_path), f"steinhardt_rank{r}.npz")) for r in range(world)]


SUMMARY_KEYS = ["n", "invalid", "mean_q4", "mean_q6", "min_q6", "min_q6_gid", "max_q6", "mean_w4", "mean_w6", "solid"]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("pot,n", [("lj5", 14), ("adams", 8)])
def test_ranks_give_the_one_rank_result(gpu, tmp_path, grid, pot, n):
    """2 and 8 ranks sharing the device (gloo transport): every rank returns the same global arrays; the NaN mask is the one-rank one, the values agree
    within the fp64 tolerances (a rank boundary is one more shifted image), the counts of the summary are equal and its means agree to 1e-12."""
    args = _cube(n) + ["-r", 0.1] + POT[pot]
    with gpu.Simulation(args) as sim:
        one = sim.steinhardt()
        s = sim.steinhardt_summary()
        solid = sim.solid_like()
    summary0 = np.array([float(s[k]) for k in SUMMARY_KEYS])
    assert np.isfinite(one).all() and one[:, 1].min() > 0.0
    got = _ranks(tmp_path, grid, args)
    for g in got:
        assert np.array_equal(g["q"], got[0]["q"]) and np.array_equal(g["summary"], got[0]["summary"]) and np.array_equal(g["solid"], got[0]["solid"])
    q, summary = got[0]["q"], got[0]["summary"]
    assert np.array_equal(np.isnan(q), np.isnan(one))
    for col in (0, 1):
        dq, dw = np.abs(q[:, col] ** 2 - one[:, col] ** 2), np.abs(q[:, 2 + col] - one[:, 2 + col])
        print(f"{grid} {pot}: l = {4 + 2 * col}: largest |difference| to one rank q^2 {dq.max():.3e} w {dw.max():.3e}")
        assert np.all(dq <= TOL64[col]) and np.all(dw <= 6.0 * TOL64[col] / one[:, col] ** 2)
    assert np.array_equal(got[0]["solid"], solid)
    for k, key in enumerate(SUMMARY_KEYS):
        if key in ("n", "invalid", "solid", "min_q6_gid"):
            assert summary[k] == summary0[k], key
        else:
            assert abs(summary[k] - summary0[k]) <= 1e-12, (key, summary[k], summary0[k])


SINGLE_RUN = """
    import numpy as np
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    sim = pkg.Simulation({args!r})
    np.savez({path!r}, pos=sim.gather(0), q=sim.steinhardt(), cutoff=sim.cutoff)
    sim.close()
    print("saved")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj5", 8), ("adams", 6)])
def test_single_precision(gpu, tmp_path, pot, n):
    """The float build (COMD_PRECISION=single) against numpy on its own gathered positions, under the fp32 rules."""
    path = str(tmp_path / "sp.npz")
    proc = _child(SINGLE_RUN.format(args=_cube(n) + ["-r", 0.1] + POT[pot], path=path), env={"COMD_PRECISION": "single"})
    assert proc.returncode == 0 and "saved" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = np.load(path)
    assert abs(float(got["cutoff"]) - RC[pot]) <= 1e-6 * RC[pot]
    ref = _numpy_steinhardt(got["pos"], n * LAT, float(got["cutoff"]), DELTA32)
    _check(got["q"], ref, single=True, what=f"single {pot}")


def _comd_hip(tmp_path, extra, ok=True):
    proc = subprocess.run([os.path.join(CSRC, "comd-hip"), "-d", os.path.join(ROOT, "pots")] + extra, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    yaml = [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]
    text = ""
    for f in yaml:
        text = (tmp_path / f).read_text()
        os.remove(tmp_path / f)
    if not ok:
        return proc, [], text
    assert proc.returncode == 0 and len(yaml) == 1, proc.stdout[-2000:] + proc.stderr[-2000:]
    rows = re.findall(r"^\s+(\d+)\s+(\d+\.\d+\s+\S+\s+\S+\s+\S+\s+\S+)\s+\S+\s+(\d+)(.*)$", proc.stdout, flags=re.M)
    return proc.stdout, rows, text


def _table(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#") and not any(line.startswith("#") for line in lines[1:])
    return lines[0], np.array([[float(x) for x in line.split()] for line in lines[1:]])


@pytest.mark.gpu
def test_comd_hip_steinhardt(gpu, tmp_path):
    hot = ["-N", "20", "-n", "10", "-T", "3000"]
    solid_at = 0.45
    with gpu.Simulation(["-x", 20, "-y", 20, "-z", 20, "-T", 3000]) as sim:
        ng = sim.n_global
        summaries = [sim.steinhardt_summary(solid_at)]
        for _ in range(2):
            sim.step(10)
            summaries.append(sim.steinhardt_summary(solid_at))
        last = sim.steinhardt()
        pos = sim.gather(0)
    assert not np.isnan(last).any()
    dump_max = float(np.median(last[:, 1]))                             # half the atoms: the dump has something to select
    # without the flag: the report of before, and no file
    out0, rows0, yaml0 = _comd_hip(tmp_path, hot)
    assert [r[0] for r in rows0] == ["0", "10", "20"]
    assert "MeanQ6" not in out0 and "Steinhardt" not in out0 and "Steinhardt" not in yaml0 and not re.search(r"^steinhardt\s", out0, flags=re.M)
    assert not re.search(r"Timer:\s+steinhardt", yaml0) and not [f for f in os.listdir(tmp_path) if f.endswith(".dat") or f.endswith(".xyz")]
    # three samples: the energies untouched to the bit, the file, the YAML block, the timer row, the dump
    out1, rows1, yaml1 = _comd_hip(tmp_path, hot + ["--steinhardt", "--stSolid", repr(solid_at), "--stFile", "x.dat", "--stDump", "d.xyz", "--stDumpMax", repr(dump_max)])
    assert [r[:3] for r in rows1] == [r[:3] for r in rows0] and "MeanQ6" in out1
    assert re.search(r"^steinhardt\s+3\s", out1, flags=re.M), out1[-3000:]
    header, table = _table(tmp_path / "x.dat")
    assert re.search(rf"\bN {ng}\b", header) and re.search(r"\bsamples 3\b", header) and abs(float(re.search(r"\bthreshold (\S+)", header).group(1)) - solid_at) <= 1e-15
    assert table.shape == (3, 11) and table[:, 0].tolist() == [0, 10, 20] and not os.path.exists(tmp_path / "steinhardt.dat")
    for row, s in zip(table, summaries):
        for k, key in enumerate(SUMMARY_KEYS):
            if key in ("n", "invalid", "solid", "min_q6_gid"):
                assert row[1 + k] == s[key], (key, row, s)
            else:
                assert abs(row[1 + k] - s[key]) <= 1e-10 * abs(s[key]), (key, row, s)
    assert [float(r[3].split()[-1]) for r in rows1] == [float(f"{row[4]:.10f}") for row in table]           # the MeanQ6 column is the last one
    block = re.search(r"^Steinhardt:\n((?:  .*\n)+)", yaml1, flags=re.M)
    assert block, yaml1[-2000:]
    m = dict(re.findall(r"^  (\w+): (\S+)$", block.group(1), flags=re.M))
    assert set(m) == {"threshold", "samples", "file", "finalMeanQ6", "finalSolidFraction"}
    assert m["samples"] == "3" and m["file"] == "x.dat" and abs(float(m["threshold"]) - solid_at) <= 1e-11
    assert abs(float(m["finalMeanQ6"]) - summaries[2]["mean_q6"]) <= 1e-10 and abs(float(m["finalSolidFraction"]) - summaries[2]["solid"] / ng) <= 1e-11
    dump = open(tmp_path / "d.xyz").read().splitlines()
    want = np.nonzero(last[:, 1] <= dump_max)[0]
    assert int(dump[0]) == len(want) == len(dump) - 2 and 0 < len(want) < ng and "Properties=species:S:1:pos:R:3:q4:R:1:q6:R:1:w4:R:1:w6:R:1:gid:I:1" in dump[1]
    atoms = [line.split() for line in dump[2:]]
    assert all(a[0] == "Cu" and len(a) == 9 for a in atoms)
    gids = np.array([int(a[8]) for a in atoms])
    assert np.array_equal(gids, want)
    assert np.array_equal(np.array([[float(x) for x in a[4:8]] for a in atoms]), last[gids])
    assert np.array_equal(np.array([[float(x) for x in a[1:4]] for a in atoms]), pos[gids])
    # refused before any step
    for bad in (["--stSolid", "0"], ["--stSolid", "1"], ["--stSolid", "-0.5"], ["--stSolid", "2"], ["--stDumpMax", "0"], ["--stDumpMax", "-1"], ["--stDumpMax", "nan"]):
        proc, _, _ = _comd_hip(tmp_path, hot + ["--steinhardt"] + bad, ok=False)
        assert proc.returncode != 0 and re.search(r"^Error:", proc.stdout, flags=re.M) and not re.search(r"^\s+0\s+0\.00\s", proc.stdout, flags=re.M), proc.stdout[-1500:]
