"""Every forced leg of the force kernels at a small shape, with proof that the leg ran -- run with `-m gpu` on an MI355X.

Most of the force code is fall-back and variant paths that only the COMD_* switches reach.  A leg test that sets a variable and compares with the
checker passes just as well when the variable never reaches the launch wrapper, or when the box never meets the leg's condition.  Every test here
therefore does two things: it compares forces, per-atom energies and (EAM) rhobar and dF/drho with the checker after a few steps, and it asserts the
leg's FACT from Simulation.force_leg_report() -- what the wrappers wrote down as they launched and what the kernels left in their small device arrays
-- or from the occupancies and positions of the run itself in numpy.  No fact is taken from the variable the test set.

The file runs in whichever precision the process is bound to (COMD_PRECISION): tests/test_single_precision.py runs every family of LEGS in the float
build, and counts the legs of a family from the same table.
"""
import json
import os
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_values.json")))
SINGLE = os.environ.get("COMD_PRECISION", "double") == "single"
TOL = G["tolerances_single" if SINGLE else "tolerances"]
TOL_SPLINE = G["tolerances_single_spline"] if SINGLE else TOL      # -P in float: the float checker is itself further from the double one (see the block's _about)

SETFL = ["-t", "setfl", "-p", "Cu01.eam.alloy"]
# Shapes: no 2-cell axis, interior cells under -a 1 (tests/test_two_cell_boxes.py runs every leg of this table again on boxes of two cells along an axis).  Occupancies
# from the checker (after 3 steps):
BOXES = {
    "lj":      dict(n=(10, 10, 11), delta=0.15, eam=0, flags=[], oracle={}),                                          # 3 x 3 x 3 cells of 126-196 atoms, 4400 atoms
    "eam":     dict(n=(8, 7, 9), delta=0.1, eam=1, flags=[], oracle={}),                                               # 5 x 5 x 6 cells of 9-18 atoms, 2016 atoms, 42-45 neighbours
    "eam_l35": dict(n=(8, 7, 9), delta=0.1, eam=1, flags=["-l", 3.5], oracle={"lat": 3.5}),                            # 5 x 4 x 6 cells of 13-23 atoms, 44-53 neighbours
    "setfl":   dict(n=(6, 7, 8), delta=0.1, eam=1, flags=SETFL, oracle={"pot_name": "Cu01.eam.alloy"}),                # 3 x 4 x 5 cells
    "long":    dict(n=(70, 5, 5), delta=0.2, eam=0, flags=["--ljCutoffSigmas", 2.5], oracle={"lj_cutoff_sigmas": 2.5}),   # 43 x 3 x 3 cells of 13-32 atoms, x up to 253 A
}

# ---- the mixed legs' values (both sides of the condition inside one launch), and what they were chosen from ----
# LJ candidate counts of the listed waves on the "lj" box: the default leg reports 845 (a tail wave of a few atoms) to 2469 (a full wave) of them after 2 steps, in
# rows of 4008 entries.  Rows of 2400 entries hold all lists but those of the five fullest waves (78 waves listed, 5 walking, the longest list kept 2306).
LJ_LIST_CAP_MIXED = 2400
# cta_cell bricks of 1 x 4 x 2 cells on the "eam" box (grid 5 x 5 x 6, 30 bricks): the blocks (3 x 6 x 4 cells) of the bricks y = 0..3 hold 918-1020 atoms, those
# of the bricks that hold the row y = 4 alone (3 x 3 x 4 cells) 486-540.  An image of 720 records holds the second kind only.
EAM_IMAGE_MIXED_CTA = 720
# thread_atom bricks: whichever shape the first launch picks on this box, 1 x 4 x 4 (blocks of 486-1530 atoms, 810 and more in 13 bricks of 20), 1 x 4 x 3 (607-1275,
# 1147 and more in 10 of 20) or 1 x 4 x 2 (as above), an image of 800 records holds part of the blocks.
EAM_IMAGE_MIXED_ATOM = 800
# round 2's cta_cell kernel: the 27-cell stencils of the "eam" box hold 324 atoms (a fifth of the cells), 360-365 or 405; a slice of 344 records holds the first kind.
EAM_STENCIL_MIXED = 344

Leg = namedtuple("Leg", "name box method flags env steps fact")


# ---------------------------------------------------------------- what the tests read from the run itself
class Ctx:
    """One leg's simulation after its steps and one more compute_force(): the report, the bricks streamed by that evaluation, and numpy views."""

    def __init__(self, sim, rep, streamed, box):
        self.sim, self.rep, self.streamed, self.box = sim, rep, streamed, box
        self._counts = None

    @property
    def counts(self):
        if self._counts is None:
            self._counts = self.sim.cells()["nAtoms"]
        return self._counts

    def stencil_sums(self):
        """atoms in the 27 cells around every local cell"""
        gx, gy, gz = self.sim.grid
        out = []
        for z in range(gz):
            for y in range(gy):
                for x in range(gx):
                    out.append(sum(int(self.counts[self.sim.box_from_tuple(x + dx, y + dy, z + dz)]) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)))
        return np.array(out)

    def block_populations(self):
        """atoms in the block (the brick's cells and the cells around them, as far as the grid with its halo reaches) of every brick of the reported shape"""
        gx, gy, gz = self.sim.grid
        by, bz = self.rep["eam_brick_shape"]
        out = []
        for z0 in range(0, gz, bz):
            for y0 in range(0, gy, by):
                for x in range(gx):
                    out.append(sum(int(self.counts[self.sim.box_from_tuple(x + dx, y, z)]) for dx in (-1, 0, 1)
                                   for y in range(y0 - 1, min(y0 + by, gy) + 1) for z in range(z0 - 1, min(z0 + bz, gz) + 1)))
        return np.array(out)

    def neighbour_counts(self):
        """atoms within the force cutoff of every atom (all pairs, minimum image)"""
        pos = self.sim.gather(0)
        lat = dict(zip(self.box["flags"][::2], self.box["flags"][1::2])).get("-l", 3.615)
        extent = np.array(self.box["n"], dtype=float) * lat
        rc2 = self.sim.cutoff ** 2
        out = np.zeros(len(pos), dtype=int)
        for s in range(0, len(pos), 512):
            d = pos[s:s + 512, None, :] - pos[None, :, :]
            d -= np.rint(d / extent) * extent
            out[s:s + 512] = ((d * d).sum(-1) <= rc2).sum(1) - 1
        return out

    def bricks_expected(self):
        gx, gy, gz = self.sim.grid
        by, bz = self.rep["eam_brick_shape"]
        return gx * -(-gy // by) * -(-gz // bz)


# ---------------------------------------------------------------- the facts
def lj_lists_all(c):
    assert c.rep["lj_lists_active"] and c.rep["lj_waves_listed"] > 0 and c.rep["lj_waves_walking"] == 0, c.rep
    assert c.rep["lj_waves_listed"] == int(((c.counts[:c.sim.n_local_boxes] + 63) // 64).sum())
    assert 0 < c.rep["lj_candidates_min"] <= c.rep["lj_candidates_max"] <= c.rep["lj_list_row_capacity"], c.rep


def lj_lists_inactive(c):
    assert not c.rep["lj_lists_active"] and c.rep["lj_waves_listed"] == 0 and c.rep["lj_waves_walking"] > 0, c.rep


def lj_rows_too_short(c):
    assert c.rep["lj_lists_active"] and c.rep["lj_list_row_capacity"] == 64 and c.rep["lj_waves_listed"] == 0 and c.rep["lj_waves_walking"] > 0, c.rep


def lj_rows_mixed(cap):
    def fact(c):
        assert c.rep["lj_lists_active"] and c.rep["lj_list_row_capacity"] == cap, c.rep
        assert c.rep["lj_waves_listed"] > 0 and c.rep["lj_waves_walking"] > 0 and c.rep["lj_candidates_max"] <= cap, c.rep
    return fact


def lj_one_wave(c):
    assert c.rep["lj_waves_per_cell"] == 1 and c.counts[:c.sim.n_local_boxes].max() > 64, (c.rep, c.counts.max())


def lj_cta_form(form):
    def fact(c):
        assert c.rep["lj_cta_form"] == form, c.rep
    return fact


def eam_kernel(kernel, cover="all_cells", extra=None):
    def fact(c):
        assert c.rep["eam_kernel"] == kernel and c.rep["eam_cover"] == cover, c.rep
        if extra:
            extra(c)
    return fact


def brick_none_streamed(c):
    assert c.streamed == 0 and c.rep["eam_bricks"] == c.bricks_expected() and c.block_populations().max() <= c.rep["eam_image_records"], (c.streamed, c.rep)
    assert not c.rep["eam_clamps_kept"] and c.rep["eam_tables_in_lds"], c.rep


def brick_all_streamed(c):
    assert c.rep["eam_image_records"] == 128 and c.block_populations().min() > 128, c.rep
    assert c.streamed == c.rep["eam_bricks"] == c.bricks_expected() > 1, (c.streamed, c.rep)


def brick_some_streamed(image):
    image = (image + 7) // 8 * 8          # (the wrappers round the image up to 8 records)

    def fact(c):
        pop = c.block_populations()
        assert c.rep["eam_image_records"] == image and pop.min() <= image < pop.max(), (c.rep, pop.min(), pop.max())
        assert 0 < c.streamed < c.rep["eam_bricks"] == c.bricks_expected(), (c.streamed, c.rep)
        assert c.streamed == int((pop > image).sum()), (c.streamed, np.sort(pop))
    return fact


def brick_shape(by, bz):
    def fact(c):
        gx, gy, gz = c.sim.grid
        assert c.rep["eam_brick_shape"] == (by, bz) and c.rep["eam_bricks"] == gx * -(-gy // by) * -(-gz // bz) == c.rep["eam_pass1_workgroups"], c.rep
    return fact


def stencil_slice(records, over):
    """round 2's cta_cell kernel: cells whose 27-cell stencil outgrows the LDS slice take the thread-per-atom form inside the kernel"""
    def fact(c):
        sums = c.stencil_sums()
        if records:
            assert c.rep["eam_stencil_records"] == records, c.rep
        frac = float((sums > c.rep["eam_stencil_records"]).mean())
        assert {"all": frac == 1.0, "some": 0.0 < frac < 1.0, "none": frac == 0.0}[over], (c.rep["eam_stencil_records"], sums.min(), sums.max())
    return fact


def clamps_kept(c):
    assert c.rep["eam_clamps_kept"], c.rep


def hand_over(on):
    def fact(c):
        assert c.rep["eam_pass3_read_rows"] == on, c.rep
        if on:
            assert c.rep["eam_row_capacity"] >= c.neighbour_counts().max(), (c.rep, c.neighbour_counts().max())
            assert c.streamed == 0 and c.rep["eam_byte_offset_limit"] == 256, (c.streamed, c.rep)
    return fact


def atom_shape(by, bz):
    def fact(c):
        assert c.rep["eam_brick_shape"] == (by, bz) and c.rep["eam_bricks"] == c.bricks_expected(), c.rep
    return fact


def rows_short_for(lo, hi):
    """the share of atoms with more neighbours than a thread's row holds"""
    def fact(c):
        frac = float((c.neighbour_counts() > c.rep["eam_row_capacity"]).mean())
        assert lo <= frac <= hi, (frac, c.rep["eam_row_capacity"])
    return fact


def rows_capacity(n, lo, hi):
    def fact(c):
        assert c.rep["eam_row_capacity"] == n, c.rep
        rows_short_for(lo, hi)(c)
    return fact


def offset_limit_64(c):
    assert c.rep["eam_byte_offset_limit"] == 64, c.rep


def nl_format(fmt, kernel=None):
    def fact(c):
        assert c.rep["neighbor_list_format"] == fmt == c.sim.force_path_info()["neighbor_list_format"] and c.sim.nl_builds >= 1, (c.rep, c.sim.nl_builds)
        if kernel:
            assert c.rep["eam_kernel"] == kernel, c.rep
    return fact


def tables(in_lds=None, spline=False):
    def fact(c):
        assert c.rep["eam_spline"] == spline, c.rep
        if in_lds is not None:
            assert c.rep["eam_tables_in_lds"] == in_lds, c.rep
    return fact


# setfl: 10000 samples per table.  Pass 1 keeps rho and phi: 2 x 10003 x sizeof(real_t) = 160 KB in double, 80 KB in float -- over the 32 KB the wrappers allow
# the tables either way (eam_launch.h EamTablePlan::tablesInLds), so both builds read them through L2; funcfl (500 samples) fits in both.
SETFL_TABLES_IN_LDS = False

A0, A1 = ["-a", 0], ["-a", 1]
LEGS = {
    "lj": [
        Leg("default", "lj", "thread_atom", [], {}, 2, lj_lists_all),
        Leg("default_interpolated", "lj", "thread_atom", ["-I"], {}, 2, lj_lists_all),
        Leg("prune_0", "lj", "thread_atom", [], {"COMD_LJ_PRUNE": "0"}, 2, lj_lists_inactive),
        Leg("budget_1mb", "lj", "thread_atom", [], {"COMD_LJ_LIST_BUDGET_MB": "1"}, 2, lj_lists_inactive),
        Leg("list_cap_64", "lj", "thread_atom", [], {"COMD_LJ_LIST_CAP": "64"}, 2, lj_rows_too_short),
        Leg("list_cap_64_interpolated", "lj", "thread_atom", ["-I"], {"COMD_LJ_LIST_CAP": "64"}, 2, lj_rows_too_short),
        Leg("list_cap_mixed", "lj", "thread_atom", [], {"COMD_LJ_LIST_CAP": str(LJ_LIST_CAP_MIXED)}, 2, lj_rows_mixed(LJ_LIST_CAP_MIXED)),
        Leg("one_wave", "lj", "thread_atom", [], {"COMD_LJ_WAVES": "1"}, 2, lj_one_wave),
        Leg("cta_boxes", "lj", "cta_cell", [], {}, 2, lj_cta_form("boxes")),
        Leg("cta_slabs", "lj", "cta_cell", [], {"COMD_LJ_CTA_SLABS": "1"}, 2, lj_cta_form("slabs")),
    ],
    "eam_cta": [
        Leg("default", "eam", "cta_cell", [], {}, 3, eam_kernel("brick", extra=brick_none_streamed)),
        Leg("image_128", "eam", "cta_cell", [], {"COMD_EAM_IMAGE": "128"}, 3, eam_kernel("brick", extra=brick_all_streamed)),
        Leg("image_mixed", "eam", "cta_cell", [], {"COMD_EAM_IMAGE": str(EAM_IMAGE_MIXED_CTA)}, 3, eam_kernel("brick", extra=brick_some_streamed(EAM_IMAGE_MIXED_CTA))),
        Leg("brick_2_2", "eam", "cta_cell", [], {"COMD_EAM_BRICK": "2,2"}, 3, eam_kernel("brick", extra=brick_shape(2, 2))),
        Leg("brick_3_5", "eam", "cta_cell", [], {"COMD_EAM_BRICK": "3,5"}, 3, eam_kernel("brick", extra=brick_shape(3, 5))),
        Leg("round2_stencil_128", "eam", "cta_cell", [], {"COMD_EAM_CTA": "cell", "COMD_EAM_STENCIL": "128"}, 3, eam_kernel("cta_cell_round2", extra=stencil_slice(128, "all"))),
        Leg("round2_stencil_mixed", "eam", "cta_cell", [], {"COMD_EAM_CTA": "cell", "COMD_EAM_STENCIL": str(EAM_STENCIL_MIXED)}, 3,
            eam_kernel("cta_cell_round2", extra=stencil_slice(EAM_STENCIL_MIXED, "some"))),
        Leg("round2_default_slice", "eam", "cta_cell", [], {"COMD_EAM_CTA": "cell"}, 3, eam_kernel("cta_cell_round2", extra=stencil_slice(0, "none"))),
        Leg("clamps_kept", "eam", "cta_cell", [], {"COMD_EAM_CLAMP": "1"}, 3, eam_kernel("brick", extra=clamps_kept)),
        Leg("overlap_whole_bricks", "eam", "cta_cell", A1, {}, 3, eam_kernel("brick", "whole_bricks")),
        Leg("overlap_groups_0", "eam", "cta_cell", A1, {"COMD_EAM_GROUPS": "0"}, 3, eam_kernel("brick", "cell_by_cell")),
    ],
    "eam_atom": [
        Leg("default", "eam", "thread_atom", A0, {}, 3, eam_kernel("atom_brick", extra=hand_over(True))),
        Leg("default_overlap", "eam", "thread_atom", A1, {}, 3, eam_kernel("atom_brick", "whole_bricks", extra=hand_over(True))),
        Leg("handover_0", "eam", "thread_atom", A0, {"COMD_EAM_ATOM_HANDOVER": "0"}, 3, eam_kernel("atom_brick", extra=hand_over(False))),
        Leg("handover_0_overlap", "eam", "thread_atom", A1, {"COMD_EAM_ATOM_HANDOVER": "0"}, 3, eam_kernel("atom_brick", "whole_bricks", extra=hand_over(False))),
        Leg("image_128", "eam", "thread_atom", A0, {"COMD_EAM_IMAGE": "128"}, 3, eam_kernel("atom_brick", extra=brick_all_streamed)),
        Leg("image_mixed", "eam", "thread_atom", A0, {"COMD_EAM_IMAGE": str(EAM_IMAGE_MIXED_ATOM)}, 3, eam_kernel("atom_brick", extra=brick_some_streamed(EAM_IMAGE_MIXED_ATOM))),
        Leg("brick_2_3", "eam", "thread_atom", A0, {"COMD_EAM_ATOM_BRICK": "2,3"}, 3, eam_kernel("atom_brick", extra=atom_shape(2, 3))),
        Leg("brick_4_5", "eam", "thread_atom", A0, {"COMD_EAM_ATOM_BRICK": "4,5"}, 3, eam_kernel("atom_brick", extra=atom_shape(4, 5))),
        Leg("rows_16", "eam", "thread_atom", A0, {"COMD_EAM_ATOM_ROWS": "16"}, 3, eam_kernel("atom_brick", extra=rows_capacity(16, 1.0, 1.0))),
        Leg("rows_48_compressed", "eam_l35", "thread_atom", A0, {"COMD_EAM_ATOM_ROWS": "48"}, 3, eam_kernel("atom_brick", extra=rows_capacity(48, 0.1, 0.9))),
        Leg("ablate_16", "eam", "thread_atom", A0, {"COMD_EAM_ABLATE": "16"}, 3, eam_kernel("atom_brick", extra=offset_limit_64)),
        Leg("round2", "eam", "thread_atom", A0, {"COMD_EAM_THREAD_ATOM": "cell"}, 3, eam_kernel("thread_atom_round2")),
        Leg("groups_0", "eam", "thread_atom", A0, {"COMD_EAM_GROUPS": "0"}, 3, eam_kernel("atom_brick", "all_cells")),
        Leg("groups_0_overlap", "eam", "thread_atom", A1, {"COMD_EAM_GROUPS": "0"}, 3, eam_kernel("atom_brick", "cell_by_cell")),
    ],
    "lists": [
        Leg("pair_slab_rows", "lj", "thread_atom_nl", [], {}, 2, nl_format(1)),
        Leg("pair_global_slots", "lj", "thread_atom_nl", [], {"COMD_NL_GLOBAL": "1"}, 2, nl_format(0)),
        Leg("eam_default", "eam", "thread_atom_nl", [], {}, 3, nl_format(4, "listed_rows")),
        Leg("eam_global", "eam", "thread_atom_nl", [], {"COMD_NL_GLOBAL": "1"}, 3, nl_format(0, "nl_global")),
        Leg("eam_nl_lds", "eam", "thread_atom_nl", [], {"COMD_EAM_NL": "lds"}, 3, nl_format(2, "nl_lds")),
    ],
    "tables": [
        Leg("setfl_thread_atom", "setfl", "thread_atom", [], {}, 3, eam_kernel("atom_brick", extra=tables(SETFL_TABLES_IN_LDS))),
        Leg("setfl_cta_cell", "setfl", "cta_cell", [], {}, 3, eam_kernel("brick", extra=tables(SETFL_TABLES_IN_LDS))),
        Leg("spline_thread_atom", "eam", "thread_atom", ["-P"], {}, 3, eam_kernel("atom_brick", extra=tables(False, True))),
        Leg("spline_cta_cell", "eam", "cta_cell", ["-P"], {}, 3, eam_kernel("brick", extra=tables(False, True))),
        Leg("spline_thread_atom_nl", "eam", "thread_atom_nl", ["-P"], {}, 3, eam_kernel("listed_rows", extra=tables(False, True))),
    ],
}
PAIRLOSS = ["thread_atom_pruned_against_walk", "cta_cell_boxes_against_slabs"]
FAMILY_LEG_COUNT = {**{family: len(legs) for family, legs in LEGS.items()}, "pairloss": len(PAIRLOSS)}      # eam_atom also runs the bit-for-bit hand-over test
FAMILY_LEG_COUNT["eam_atom"] += 1


# ---------------------------------------------------------------- the checker's answer, computed once per (box, steps, capacity, tables)
_REFERENCE = {}


def _reference(orc, key, steps, cap, spline):
    k = (key, steps, cap, spline)
    if k not in _REFERENCE:
        box = BOXES[key]
        o = orc.Oracle(box["n"], eam=box["eam"], delta=box["delta"], cap=cap, spline=spline, **box["oracle"])
        o.step(steps)
        got = {"f": o.gather(orc.F), "u": o.gather(orc.U)}
        if box["eam"]:
            got.update(rho=o.gather(orc.RHOBAR), df=o.gather(orc.DFEMBED))
        for v in got.values():
            v.setflags(write=False)
        o.close()
        _REFERENCE[k] = got
    return _REFERENCE[k]


def _args(box, method, flags):
    nx, ny, nz = box["n"]
    return ["-x", nx, "-y", ny, "-z", nz, "-r", box["delta"], "-m", method] + (["-e"] if box["eam"] else []) + list(box["flags"]) + list(flags)


def _run_leg(gpu, orc, monkeypatch, leg):
    for k, v in leg.env.items():
        monkeypatch.setenv(k, v)
    box = BOXES[leg.box]
    with gpu.Simulation(_args(box, leg.method, leg.flags)) as sim:
        sim.step(leg.steps)
        f, u = sim.gather(2), sim.gather(3)
        spline = "-P" in leg.flags
        tol = TOL_SPLINE if spline else TOL
        if "-I" in leg.flags:       # the checker has no -I: the restatement of tests/test_lj_interpolation.py at the positions of this run
            from test_lj_interpolation import LAT, SIGMA, lj_table, restated_forces
            fo, uo = restated_forces(sim.gather(0), np.array(box["n"], dtype=float) * LAT, lj_table(), 5.0 * SIGMA)
            ref = {"f": fo, "u": uo}
        else:
            ref = _reference(orc, leg.box, leg.steps, max(sim.max_atoms, 64), spline)
        err = {"f": np.abs(f - ref["f"]).max() / np.abs(ref["f"]).max(), "u": np.abs(u - ref["u"]).max()}
        if box["eam"]:
            err.update(rho=np.abs(sim.gather(4) - ref["rho"]).max(), df=np.abs(sim.gather(5) - ref["df"]).max())
        print(f"{leg.box} {leg.method} {leg.name}: " + "  ".join(f"{k} {v:.3e}" for k, v in err.items()))
        assert err["f"] <= tol["force_rel_to_max"] and err["u"] <= tol["per_atom_energy_abs"], err
        if box["eam"]:
            assert err["rho"] < tol["eam_density_abs"] and err["df"] < tol["eam_dfembed_abs"], err
        leg.fact(observe(sim, box))


def observe(sim, box):
    """One more force evaluation of the state `sim` is in, and what it ran: the report, and the bricks that evaluation streamed (the count is cumulative)."""
    before = sim.force_leg_report()
    sim.redistribute()      # (-a 1 launches the interior cells' passes 1 and 2 here)
    sim.compute_force()
    rep = sim.force_leg_report()
    print(rep)
    return Ctx(sim, rep, rep["eam_bricks_streamed_total"] - before["eam_bricks_streamed_total"], box)


def _ids(family):
    return dict(argnames="leg", argvalues=LEGS[family], ids=[leg.name for leg in LEGS[family]])


@pytest.mark.parametrize(**_ids("lj"))
def test_lj_leg(gpu, orc, monkeypatch, leg):
    """LJ thread_atom: candidate lists, the 27-cell walk they fall back to, both inside one launch, extra chunks of a cell with one wave; cta_cell in both forms."""
    _run_leg(gpu, orc, monkeypatch, leg)


@pytest.mark.parametrize(**_ids("eam_cta"))
def test_eam_cta_leg(gpu, orc, monkeypatch, leg):
    """EAM cta_cell: the brick image and its streaming form, brick shapes, round 2's kernel and its slice overflow, kept clamps, the overlap mode's two covers."""
    _run_leg(gpu, orc, monkeypatch, leg)


@pytest.mark.parametrize(**_ids("eam_atom"))
def test_eam_atom_leg(gpu, orc, monkeypatch, leg):
    """EAM thread_atom on the brick image: the hand-over of rows, the streaming form, brick shapes, rows that overflow, runs too long for byte offsets, round 2's kernel."""
    _run_leg(gpu, orc, monkeypatch, leg)


def test_eam_atom_hand_over_changes_no_bit(gpu, monkeypatch):
    """What pass 3 reads from pass 1's rows is what its own test finds, in the same order: forces and energies with and without the hand-over agree to the last
    bit, on one launch per pass and under -a 1 with the lists taken cell by cell (bricks staged under two selections).

    In the float build this did not hold before EAM_Force_atom_brick fixed its contraction mode (eam_atom_brick_kernels.h, #pragma clang fp contract(on)): 1099 of these
    2016 atoms differed in a force component by up to 1.07e-6 eV/A (max|f| 1.74), with equal energies -- the optimiser had fused other products in the copy of the pair
    arithmetic that reads rows from registers than in the copy that reads them from the LDS."""
    box, got = BOXES["eam"], []
    monkeypatch.setenv("COMD_EAM_GROUPS", "0")
    for handover, overlap in (("1", 0), ("0", 0), ("1", 1), ("0", 1)):
        monkeypatch.setenv("COMD_EAM_ATOM_HANDOVER", handover)
        with gpu.Simulation(_args(box, "thread_atom", ["-a", overlap])) as sim:
            sim.step(3)
            rep = sim.force_leg_report()
            assert rep["eam_kernel"] == "atom_brick" and rep["eam_pass3_read_rows"] == (handover == "1"), rep
            assert rep["eam_cover"] == ("cell_by_cell" if overlap else "all_cells"), rep
            got.append((sim.gather(2).copy(), sim.gather(3).copy()))
    for k in (0, 2):
        assert np.array_equal(got[k][0], got[k + 1][0]) and np.array_equal(got[k][1], got[k + 1][1])


@pytest.mark.parametrize(**_ids("lists"))
def test_lists_leg(gpu, orc, monkeypatch, leg):
    """thread_atom_nl: Verlet rows in the LJ slab format, the EAM brick rows, round 3's LDS lists and the global-slot format."""
    _run_leg(gpu, orc, monkeypatch, leg)


@pytest.mark.parametrize(**_ids("tables"))
def test_tables_leg(gpu, orc, monkeypatch, leg):
    """setfl tables (10000 samples: behind L2 in both precisions) and the cubic-spline tables of -P on every method."""
    _run_leg(gpu, orc, monkeypatch, leg)


# ---------------------------------------------------------------- a pair lost at the cutoff, at a size a float run can see
# One pair at the unshifted LJ force cutoff r_c = 2.5 sigma is a jump of J = (24 eps / r_c) (sigma / r_c)^6 (1 - 2 (sigma / r_c)^6) = 2.81e-3 eV/A; the order of
# summation moves a force by about eps_machine * sum |f_ij|, below 1e-5 eV/A in float with max|f| = 14 eV/A.  The bound J / 10 has 10x room on either side.
_S6 = 2.5 ** -6
PAIR_JUMP = 24.0 * 0.167 / (2.5 * 2.315) * _S6 * (1.0 - 2.0 * _S6)


@pytest.mark.parametrize("which", PAIRLOSS)
def test_pairloss(gpu, monkeypatch, which):
    """The two pruned LJ forms against their unpruned forms on a long box (x up to 253 A, where a float ulp is 1.5e-5 A): the list build of thread_atom
    prunes in fp32 with margins (comd_device.hip ljBoxMarginsF), cta_cell's default form prunes by boxes (ljBoxMargins).  Neither may lose a pair.  No
    checker on this box: the float and double checkers themselves differ by more than the float energy bound here."""
    assert abs(PAIR_JUMP - 2.81e-3) < 1e-5
    method, name, values, form = {"thread_atom_pruned_against_walk": ("thread_atom", "COMD_LJ_PRUNE", ("1", "0"), None),
                                  "cta_cell_boxes_against_slabs": ("cta_cell", "COMD_LJ_CTA_SLABS", ("0", "1"), ("boxes", "slabs"))}[which]
    box, out = BOXES["long"], []
    for k, value in enumerate(values):
        monkeypatch.setenv(name, value)
        with gpu.Simulation(_args(box, method, [])) as sim:
            sim.step(2)
            out.append(sim.gather(2).copy())
            rep = sim.force_leg_report()
            if method == "thread_atom":
                assert rep["lj_lists_active"] == (k == 0), rep
                assert k == 1 or (rep["lj_waves_listed"] > 0 and rep["lj_waves_walking"] == 0), rep
            else:
                assert rep["lj_cta_form"] == form[k], rep
    diff = np.abs(out[0] - out[1]).max()
    print(f"{which}: max|df| {diff:.3e} eV/A, bound {PAIR_JUMP / 10:.3e}, max|f| {np.abs(out[0]).max():.3f}")
    assert np.abs(out[0]).max() > 1.0 and diff < PAIR_JUMP / 10
