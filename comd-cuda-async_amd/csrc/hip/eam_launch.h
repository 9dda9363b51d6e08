// eam_launch.h -- the EAM launch layer: which kernel a force pass runs on, and the sizes it is launched with.  Host code, part of comd_device.hip's translation unit (it uses
// HIP_CHECK, ForceTimer, dalloc, allowDynamicLds, nlView, tuningOf and latticeConstantOf of that file).  Pass 1 and pass 3 of a force evaluation must size tables, rows and
// images alike, so every such rule is written once here.
#pragma once

static EamArgs makeEamArgs(SimGpu* sim, int num_cells, int* cells_list)
{
   EamArgs a;
   a.rx = sim->atoms.r.x; a.ry = sim->atoms.r.y; a.rz = sim->atoms.r.z;
   a.fx = sim->atoms.f.x; a.fy = sim->atoms.f.y; a.fz = sim->atoms.f.z; a.e = sim->atoms.e;
   a.rhobar = sim->eam_pot.rhobar; a.dfEmbed = sim->eam_pot.dfEmbed;
   a.nAtoms = sim->boxes.nAtoms; a.nbr = sim->neighbor_cells; a.cells = cells_list;
   a.nCells = num_cells; a.cap = sim->maxAtoms;
   a.rc2 = sim->eam_pot.cutoff * sim->eam_pot.cutoff;
   a.phi = sim->eam_pot.phi; a.rho = sim->eam_pot.rho; a.f = sim->eam_pot.f;
   a.phiS = sim->eam_pot.phiS; a.rhoS = sim->eam_pot.rhoS;
   a.sel = nullptr; a.tag = 0;
   return a;
}

// The rho / phi tables of a pass (step 1: both, step 3: rho; step 0, the list build, reads none) and where they live: funcfl tables (500 samples) in the LDS,
// setfl tables (10000) and the spline coefficients of -P behind L2.
struct EamTablePlan {
   InterpolationObjectGpu phi, rho;
   bool spline, sameGrid;                                    // sameGrid: phi and rho share a grid (one index per pair, one copy of the grid)
   EamTablePlan(const InterpolationObjectGpu& phi_, const InterpolationObjectGpu& rho_, int spline_)
      : phi(phi_), rho(rho_), spline(spline_ != 0), sameGrid(phi_.n == rho_.n && phi_.x0 == rho_.x0 && phi_.invDx == rho_.invDx) {}
   size_t tableBytes(int step) const { return eamCtaTableBytes(step, rho.n, phi.n); }
   bool tablesInLds(int step) const { return step != 0 && !spline && tableBytes(step) <= 32 * 1024; }
   size_t tableDoubles(int step) const                       // table entries a brick kernel keeps in the LDS
   { return !tablesInLds(step) ? 0 : step == 1 ? (size_t)2 * (rho.n + 3) + (sameGrid ? 0 : (phi.n + 3 - (rho.n + 3))) : (size_t)(rho.n + 3); }
};

// rows per atom: the atoms inside the cutoff sphere at the lattice's density, times `factor`, a multiple of 8 within [lo, hi]
static int eamRowsPerAtom(const SimGpu* sim, double factor, int lo, int hi)
{
   const double rc = sim->eam_pot.cutoff, lat = latticeConstantOf(sim);
   const int rows = ((int)(SPHERE_VOLUME * rc * rc * rc * 4.0 / (lat * lat * lat) * factor) + 7) / 8 * 8;
   return rows < lo ? lo : rows > hi ? hi : rows;
}
// The volume of a link cell AS ALLOCATED (AllocateGpu), not the current one: everything sized from it -- row threads and with them the stride of the row buffers of
// thread_atom, LDS slices, the first guess of an image -- is an estimate of how many atoms a cell holds, and a box remapped by comdRemapBoxGpu stretches its cells WITH
// their atoms.  Derived from the current volume, the row stride of launchEamAtomBrick changed under a stretched box while its buffers kept the stride they were allocated with.
static double eamCellVolume(const SimGpu* sim) { return sim->cellVolume0; }
// a launch with dynamic LDS: the size is allowed for the kernel first
template <typename... P, typename... A>
static void launchLds(void (*kernel)(P...), int grid, int threads, size_t lds, hipStream_t st, const A&... args)
{ allowDynamicLds((const void*)kernel, lds); hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, st, args...); }
// workgroups of `bytes` of LDS that share a CU: 160 KB, handed out in 1280-byte granules
static int ldsWorkgroupsPerCu(size_t bytes) { return bytes > 160 * 1024 ? 0 : (int)(160 * 1024 / (((bytes + 1279) / 1280) * 1280)); }

// The table clamps of interpolate() are dead weight when every pair the kernel evaluates lies inside the tables: 0 < r <= cutoff (rows hold pairs inside the cutoff;
// listed pairs are evaluated at min(r, cutoff)), tables from x0 <= 0 up to xn >= cutoff.  COMD_EAM_CLAMP=1 keeps them (A/B runs).
static bool eamClampFree(SimGpu* sim, const EamArgs& a, int spline)
{
   const double rcut = sim->eam_pot.cutoff * (1.0 + 4e-16);
   return !spline && a.phi.x0 <= R(0.0) && a.rho.x0 <= R(0.0) && rcut <= (double)a.phi.xn && rcut <= (double)a.rho.xn && !tuningOf(sim).eamClamp;
}

// cta_cell, brick form (eam_brick_kernels.h): a workgroup stages the cells around a brick of 1 x BY x BZ cells once and its waves take the
// brick's cells one at a time.  COMD_EAM_BRICK="by,bz" overrides the brick (experiments).  The Verlet-list method of EAM (slabFormat 4) runs on the
// same kernel with LISTED = true: rows built once per list build, both passes read them back.
static bool eamArraysBelow4GiB(const SimGpu* sim) { return (double)sim->boxes.nTotalBoxes * sim->maxAtoms * sizeof(real_t) < 4294967296.0; }      // (the brick kernels stage with 32-bit byte offsets)
static bool eamListedBrick(const SimGpu* sim, int method) { return (method == THREAD_ATOM_NL || method == WARP_ATOM_NL) && sim->atoms.neighborList.slabFormat == 4; }
static bool eamBrickPath(SimGpu* sim, int method) { return eamListedBrick(sim, method) || (method == CTA_CELL && !tuningOf(sim).eamCtaCell && eamArraysBelow4GiB(sim)); }
// thread_atom on the brick image (eam_atom_brick_kernels.h).  COMD_EAM_THREAD_ATOM=cell keeps round 2's kernel (a share of a wave per cell, candidates streamed
// through L2; A/B runs), as do arrays of 4 GiB or more.
static bool eamAtomBrickPath(SimGpu* sim, int method) { return (method == THREAD_ATOM || method == WARP_ATOM) && !tuningOf(sim).eamThreadAtomCell && eamArraysBelow4GiB(sim); }
// The overlap mode's two lists as brick groups (eam_brick_kernels.h ClassifyBrickCells): 1 = this is the launch over SimGpu.boundary_cells, 2 = over
// SimGpu.interior_cells, 0 = any other list (cell marks).  COMD_EAM_GROUPS=0 keeps the lists as they are given (A/B runs, tests).
static int eamBrickGroupOf(SimGpu* sim, const int* cells_list, int num_cells, int method)
{
   if (!cells_list || !(eamBrickPath(sim, method) || eamAtomBrickPath(sim, method))) return 0;
   if (!tuningOf(sim).eamGroups) return 0;
   if (cells_list == sim->boundary_cells && num_cells == sim->n_boundary_cells) return 1;
   if (cells_list == sim->interior_cells && num_cells == sim->n_interior_cells) return 2;
   return 0;
}

static void eamBrickGeometry(const SimGpu* sim, EamBrickArgs* b)
{
   memset(b, 0, sizeof *b);
   for (int k = 0; k < 3; ++k) { b->geom.g[k] = sim->boxes.gridSize[k]; b->geom.lmin[k] = sim->boxes.localMin[k]; b->geom.lmax[k] = sim->boxes.localMax[k]; b->geom.inv[k] = sim->boxes.invBoxSize[k]; }
   b->geom.nLocal = sim->boxes.nLocalBoxes; b->geom.nTotal = sim->boxes.nTotalBoxes;
   b->geom.lookup = sim->boxes.boxIDLookUp; b->geom.reverse = sim->boxes.boxIDLookUpReverse;
}
static void eamBrickSetShape(EamBrickArgs* b, int by, int bz) { b->by = by; b->bz = bz; b->nby = ceilDiv(b->geom.g[1], by); b->nbz = ceilDiv(b->geom.g[2], bz); }
static int eamBrickCount(const EamBrickArgs& b) { return b.geom.g[0] * b.nby * b.nbz; }

// The brick shape of cta_cell and of the list method: 1 x 4 x 2 cells unless COMD_EAM_BRICK says otherwise; fixed by the first launch (rows index the image of that shape).
static void eamBrickOwnShape(SimGpu* sim, bool listed, EamBrickArgs* b)
{
   if (!sim->eam_pot.brickBy) {
      const ComdTuning& t = tuningOf(sim);
      const int maxCells = listed ? (EAM_BRICK_STAGE_LISTED * 256) / 32 : EAM_BRICK_MAX_CELLS;      // what the staging loop covers (eam_brick_kernels.h)
      const bool forced = t.eamBrickBy && 3 * (t.eamBrickBy + 2) * (t.eamBrickBz + 2) <= maxCells;
      sim->eam_pot.brickBy = forced ? t.eamBrickBy : 4; sim->eam_pot.brickBz = forced ? t.eamBrickBz : 2;
   }
   eamBrickSetShape(b, sim->eam_pot.brickBy, sim->eam_pot.brickBz);
}

// The host's look at the cell occupancies: counts and cell numbering read back once (this blocks on `st`, and completes whatever else the caller has queued there),
// and the atoms of the three x cells around every (x, y, z), y and z from -1 to g -- the rows a brick's block is made of.
struct EamOccupancy {
   CellGeom hg;                                              // the geometry with the numbering on the host (points into `lookup`: no copies)
   int gx, gy, gz;
   std::vector<int> counts, lookup, row3;
   EamOccupancy(SimGpu* sim, const CellGeom& geom, hipStream_t st)
      : hg(geom), gx(geom.g[0]), gy(geom.g[1]), gz(geom.g[2]), counts((size_t)sim->boxes.nTotalBoxes), row3((size_t)gx * (gy + 2) * (gz + 2))
   {
      HIP_CHECK(hipMemcpyAsync(counts.data(), sim->boxes.nAtoms, counts.size() * sizeof(int), hipMemcpyDeviceToHost, st));
      if (sim->boxes.boxIDLookUp) {
         lookup.resize((size_t)sim->boxes.nLocalBoxes);
         HIP_CHECK(hipMemcpyAsync(lookup.data(), sim->boxes.boxIDLookUp, lookup.size() * sizeof(int), hipMemcpyDeviceToHost, st));
      }
      HIP_CHECK(hipStreamSynchronize(st));
      hg.lookup = lookup.empty() ? nullptr : lookup.data(); hg.reverse = nullptr;
      for (int z = -1; z <= gz; ++z) for (int y = -1; y <= gy; ++y) for (int x = 0; x < gx; ++x)
         row3[index(x, y, z)] = counts[comdBoxFromTuple(&hg, x - 1, y, z)] + counts[comdBoxFromTuple(&hg, x, y, z)] + counts[comdBoxFromTuple(&hg, x + 1, y, z)];
   }
   EamOccupancy(const EamOccupancy&) = delete;
   size_t index(int x, int y, int z) const { return (size_t)x + (size_t)gx * ((y + 1) + (size_t)(gy + 2) * (z + 1)); }
   int cell(int x, int y, int z) const { return comdBoxFromTuple(&hg, x, y, z); }
   // records in the image of the brick part [z0, z0 + nz) of brick (x, byI, .): the kernel stages rows y0-1 .. y0+by and planes z0-1 .. z0+nz that lie inside -1 .. g
   long blockAtoms(const EamBrickArgs& b, int x, int byI, int z0, int nz) const
   {
      long sum = 0;
      for (int z = z0 - 1; z <= z0 + nz && z <= gz; ++z) for (int y = byI * b.by - 1; y <= byI * b.by + b.by && y <= gy; ++y) sum += row3[index(x, y, z)];
      return sum;
   }
};

// The image must hold the atoms of the fullest BLOCK (3 x (by + 2) x (bz + 2) cells), not the mean: the lattice and the cell grid are incommensurate,
// and at 80^3 the blocks of a 1 x 4 x 2 brick hold 755 atoms on average and up to 918.  A brick whose block outgrows the image takes the
// thread-per-atom form (correct, many times slower), so the occupancies are read once, the fullest block of this brick shape is found and the image
// sized for it + 1 % + 8 (blocks gain or lose a handful of atoms through their surface as the lattice moves).  Both passes use that size.
// Called by the first launch, and again when comdEamBrickStats finds bricks in the fall-back (comdEamBrickResize).
static int eamBrickSizeImage(SimGpu* sim, const EamBrickArgs& b, hipStream_t st, bool listed)
{
   const EamOccupancy occ(sim, b.geom, st);
   // (only blocks made of local cells count: with -a 1 the first launch runs while the halo cells are still being filled; the lattice is periodic, the
   // blocks at the faces are no fuller than those inside.  A grid too small to have such blocks takes the mean density + 25 %.)
   long fullest = 0;
   for (int bzI = 0; bzI < b.nbz; ++bzI) for (int byI = 0; byI < b.nby; ++byI) for (int x = 1; x < occ.gx - 1; ++x) {
      if (byI * b.by - 1 < 0 || byI * b.by + b.by > occ.gy - 1 || bzI * b.bz - 1 < 0 || bzI * b.bz + b.bz > occ.gz - 1) continue;
      const long sum = occ.blockAtoms(b, x, byI, bzI * b.bz, b.bz);
      if (sum > fullest) fullest = sum;
   }
   const double lat = latticeConstantOf(sim);
   if (fullest == 0) fullest = (long)(1.25 * 3 * (b.by + 2) * (b.bz + 2) * eamCellVolume(sim) * 4.0 / (lat * lat * lat));
   int cap = (((int)(fullest * 1.01) + 8 + (listed ? 1 : 0) + 7) / 8) * 8;      // (listed launches keep one more record: the far-away one that pads odd rows)
   if (cap < 256) cap = 256;
   if (cap > 4096) cap = 4096;                            // 16-bit numbers would reach 65535; beyond 4096 records the cells take the thread-per-atom form
   if (tuningOf(sim).eamImage) cap = tuningOf(sim).eamImage;      // experiments / tests: force the fallback
   return cap;
}

// Verlet rows: the brick lists of a list build.  The occupancies are final (the atom exchange has run) and frozen until the next build, so the host can
// look at every block once: the image is sized for what the passes can keep four workgroups per CU with, a brick whose block would outgrow it is listed as
// its two z halves (eam_brick_kernels.h), and the boundary / interior launches of the overlap mode get their lists of whole bricks here as well.
static void eamBrickBuildLists(SimGpu* sim, hipStream_t st, int spline)
{
   NeighborListGpu* n = &sim->atoms.neighborList;
   EamBrickArgs b;
   eamBrickGeometry(sim, &b); eamBrickOwnShape(sim, true, &b);
   const int gx = b.geom.g[0], gy = b.geom.g[1], gz = b.geom.g[2], nBricks = eamBrickCount(b);
   std::vector<int> boundary((size_t)(sim->boundary_cells ? sim->n_boundary_cells : 0));
   if (!boundary.empty()) HIP_CHECK(hipMemcpyAsync(boundary.data(), sim->boundary_cells, boundary.size() * sizeof(int), hipMemcpyDeviceToHost, st));
   const EamOccupancy occ(sim, b.geom, st);
   std::vector<long> whole((size_t)nBricks);
   long fullest = 0;
   for (int i = 0; i < nBricks; ++i) {
      const int x = i % gx, byI = (i / gx) % b.nby, bzI = i / (gx * b.nby);
      whole[i] = occ.blockAtoms(b, x, byI, bzI * b.bz, b.bz);
      if (whole[i] > fullest) fullest = whole[i];
   }
   // the largest image that leaves four workgroups per CU in pass 1 and in pass 3
   const int waves = 4;
   const EamTablePlan plan(sim->eam_pot.phi, sim->eam_pot.rho, spline);
   auto perCu = [&](int step, int cap) { return ldsWorkgroupsPerCu(eamBrickLdsBytes(step, true, plan.tableDoubles(step), cap, n->brickRowLen, waves)); };
   int cap = (((int)fullest + 1 + 7) / 8) * 8;                // (+ 1: the far-away record; nothing moves between builds, so no head-room)
   if (cap < 256) cap = 256;
   if (cap <= 4096 && (perCu(1, cap) < 4 || perCu(3, cap) < 4) && b.bz % 2 == 0) {
      int fit = cap;
      while (fit > 256 && (perCu(1, fit) < 4 || perCu(3, fit) < 4)) fit -= 8;
      long split = 0; for (int i = 0; i < nBricks; ++i) split += whole[i] + 1 > fit;
      if (split * 10 <= nBricks) cap = fit;                  // worth it while at most one brick in ten is staged twice
   }
   if (cap > 4096) cap = 4096;
   if (tuningOf(sim).eamImage) cap = tuningOf(sim).eamImage;      // experiments / tests: force halves and the fall-back
   sim->eam_pot.brickImageCap = cap;
   const int headroom = cap / 32 > 8 ? cap / 32 : 8;
   // the lists: [0, stride) bricks that hold a boundary cell, [stride, 2 stride) the others, [2 stride, 3 stride) all of them; brick order, halves adjacent
   std::vector<char> isBoundary((size_t)sim->boxes.nLocalBoxes, 0);
   for (int c : boundary) if (c >= 0 && c < sim->boxes.nLocalBoxes) isBoundary[c] = 1;
   const int stride = 2 * nBricks;
   std::vector<int> lists((size_t)3 * stride, 0), group((size_t)sim->boxes.nLocalBoxes, 2);
   int cnt[3] = { 0, 0, 0 };
   for (int i = 0; i < nBricks; ++i) {
      const int x = i % gx, by0 = ((i / gx) % b.nby) * b.by, bz0 = (i / (gx * b.nby)) * b.bz;
      bool any = false;
      for (int dz = 0; dz < b.bz; ++dz) for (int dy = 0; dy < b.by; ++dy)
         if (by0 + dy < gy && bz0 + dz < gz) any = any || isBoundary[occ.cell(x, by0 + dy, bz0 + dz)];
      for (int dz = 0; dz < b.bz; ++dz) for (int dy = 0; dy < b.by; ++dy)
         if (by0 + dy < gy && bz0 + dz < gz) group[occ.cell(x, by0 + dy, bz0 + dz)] = any ? 1 : 2;
      const int g = any ? 0 : 1;
      // (a brick within 3 % of the image goes in halves too: the lists outlive this build -- atoms wander between cells from one build to the next -- and a brick
      // that outgrows the image later takes the thread-per-atom form until the lists are made again)
      const bool halves = whole[i] + 1 > cap - headroom && b.bz % 2 == 0 && bz0 + b.bz / 2 < gz;      // (an upper half outside the grid would be an empty workgroup)
      const int e[2] = { halves ? i | (1 << 28) : i, i | (2 << 28) };
      for (int k = 0; k < (halves ? 2 : 1); ++k) { lists[(size_t)g * stride + cnt[g]++] = e[k]; lists[(size_t)2 * stride + cnt[2]++] = e[k]; }
   }
   if (sim->eam_pot.brickList && sim->eam_pot.brickListStride != stride) { HIP_CHECK(hipFree(sim->eam_pot.brickList)); sim->eam_pot.brickList = nullptr; }
   if (!sim->eam_pot.brickList) sim->eam_pot.brickList = dalloc<int>((size_t)3 * stride, false);
   if (!sim->eam_pot.brickGroup) sim->eam_pot.brickGroup = dalloc<int>((size_t)sim->boxes.nLocalBoxes, false);
   HIP_CHECK(hipMemcpyAsync(sim->eam_pot.brickList, lists.data(), lists.size() * sizeof(int), hipMemcpyHostToDevice, st));
   HIP_CHECK(hipMemcpyAsync(sim->eam_pot.brickGroup, group.data(), group.size() * sizeof(int), hipMemcpyHostToDevice, st));
   HIP_CHECK(hipStreamSynchronize(st));                      // (the vectors go out of scope; the other stream of the overlap mode reads the lists too)
   sim->eam_pot.brickCount[0] = cnt[0]; sim->eam_pot.brickCount[1] = cnt[1]; sim->eam_pot.brickCountAll = cnt[2]; sim->eam_pot.brickListStride = stride;
   sim->eam_pot.brickGroupBy = b.by; sim->eam_pot.brickGroupBz = b.bz; sim->eam_pot.brickListMakes++;
}

// The marks of a launch over an arbitrary cell list, allocated by the first such launch and zeroed ON THE LAUNCH STREAM: hipMemset returns before the
// device has finished, and the -a 1 streams are non-blocking -- a zeroing on the null stream can land after the marks of the first launch (seen once in
// four-rank runs: a first force evaluation that skipped cells).
static int* eamCellMarks(SimGpu* sim, hipStream_t st)
{
   if (sim->eam_pot.cellSel) return sim->eam_pot.cellSel;
   sim->eam_pot.cellSel = dalloc<int>((size_t)sim->boxes.nLocalBoxes, false);
   HIP_CHECK(hipMemsetAsync(sim->eam_pot.cellSel, 0, (size_t)sim->boxes.nLocalBoxes * sizeof(int), st));
   return sim->eam_pot.cellSel;
}
// A launch over any cell list that is not a brick group: mark the cells under a fresh tag, every brick looks at its own
static void eamSelectCells(SimGpu* sim, const int* cells_list, int num_cells, hipStream_t st, EamBrickArgs* b)
{
   int* marks = eamCellMarks(sim, st);
   b->sel = marks; b->tag = ++sim->eam_pot.selTag;
   ForceTimer aux(sim, st, 1);
   hipLaunchKernelGGL(MarkCells, dim3(ceilDiv(num_cells, 256)), dim3(256), 0, st, cells_list, num_cells, marks, b->tag);
}

// The bricks of the boundary and of the interior launch as lists, for the brick shape in `b` (built once per shape; eam_pot.brickGroup marks the cells for
// kernels over cells).  Shared by cta_cell and thread_atom on the brick image.
static void eamBrickGroupLists(SimGpu* sim, const EamBrickArgs& b, hipStream_t st)
{
   if (sim->eam_pot.brickGroup && sim->eam_pot.brickGroupBy == b.by && sim->eam_pot.brickGroupBz == b.bz) return;
   if (!sim->eam_pot.brickGroup) sim->eam_pot.brickGroup = dalloc<int>((size_t)sim->boxes.nLocalBoxes, false);
   int* marks = eamCellMarks(sim, st);
   const int tag = ++sim->eam_pot.selTag;
   if (sim->n_boundary_cells > 0)
      hipLaunchKernelGGL(MarkCells, dim3(ceilDiv(sim->n_boundary_cells, 256)), dim3(256), 0, st, sim->boundary_cells, sim->n_boundary_cells, marks, tag);
   const int nBricks = eamBrickCount(b);
   if (sim->eam_pot.brickList) HIP_CHECK(hipFree(sim->eam_pot.brickList));
   sim->eam_pot.brickList = dalloc<int>((size_t)2 * nBricks, false);
   hipLaunchKernelGGL(ClassifyBrickCells, dim3(ceilDiv(nBricks, 256)), dim3(256), 0, st, b, marks, tag, sim->eam_pot.brickGroup, sim->eam_pot.brickList);
   // the bricks of either group as a list (built once; the other stream of the overlap mode reads groups and lists too, so wait here):
   // [0, n1) the bricks that hold a boundary cell, [nBricks, nBricks + n2) the others, each in brick order
   std::vector<int> cls((size_t)nBricks), lists((size_t)2 * nBricks, 0);
   HIP_CHECK(hipMemcpyAsync(cls.data(), sim->eam_pot.brickList, (size_t)nBricks * sizeof(int), hipMemcpyDeviceToHost, st));
   HIP_CHECK(hipStreamSynchronize(st));
   int n1 = 0, n2 = 0;
   for (int i = 0; i < nBricks; ++i) { if (cls[i] == 1) lists[n1++] = i; else lists[(size_t)nBricks + n2++] = i; }
   HIP_CHECK(hipMemcpyAsync(sim->eam_pot.brickList, lists.data(), lists.size() * sizeof(int), hipMemcpyHostToDevice, st));
   HIP_CHECK(hipStreamSynchronize(st));
   sim->eam_pot.brickCount[0] = n1; sim->eam_pot.brickCount[1] = n2; sim->eam_pot.brickListStride = nBricks;
   sim->eam_pot.brickGroupBy = b.by; sim->eam_pot.brickGroupBz = b.bz;
}

// What the brick launchers share behind their shape and rows: the statistics, the switches, and which bricks or cells of `cells_list` the launch covers.  Returns the grid.
static int eamBrickCover(SimGpu* sim, EamBrickArgs* b, int num_cells, int* cells_list, hipStream_t st, bool listed, int method)
{
   if (!sim->eam_pot.brickStats) sim->eam_pot.brickStats = dalloc<int>(3);
   b->stats = sim->eam_pot.brickStats; b->fuseEmbed = sim->fuseEmbed; b->status = sim->status; b->debug = tuningOf(sim).eamAblate;
   const int group = eamBrickGroupOf(sim, cells_list, num_cells, method);
   if (listed) {           // the lists of the last list build (eamBrickBuildLists): all bricks, or the whole bricks of the boundary / interior launch
      if (!sim->eam_pot.brickList) { fprintf(stderr, "eamForce: thread_atom_nl needs buildNeighborListGpu before the first force call\n"); exit(-1); }
      b->brickList = sim->eam_pot.brickList + (size_t)(group ? group - 1 : 2) * sim->eam_pot.brickListStride;
   }
   if (group && !listed) {            // the boundary / interior launch of the overlap mode: whole bricks (a brick with cells of both lists would be staged twice per pass)
      eamBrickGroupLists(sim, *b, st);
      // every cell of a listed brick is selected: no marks to look at (the embedding pass, a kernel over cells, uses brickGroup)
      b->brickList = sim->eam_pot.brickList + (group == 1 ? 0 : sim->eam_pot.brickListStride);
   } else if (cells_list && !group) eamSelectCells(sim, cells_list, num_cells, st, b);
   ForceLegs& legs = legsOf(sim);
   legs.eamCover = group ? 1 : cells_list ? 2 : 0; legs.eamBy = b->by; legs.eamBz = b->bz; legs.eamBricks = eamBrickCount(*b); legs.eamRunMax = (b->debug & 16) ? 64 : 256;
   return group ? sim->eam_pot.brickCount[group - 1] : listed ? sim->eam_pot.brickCountAll : eamBrickCount(*b);
}

// thread per atom: lanes per cell = the fullest cell the host has seen (+ 2), as a power of two; persistent workgroups when the tables
// sit in the LDS (8 per CU's worth of 256 CUs), one workgroup per 256 / lanesPerCell cells otherwise
template <int STEP>
static void launchEamThreadAtom(SimGpu* sim, const EamArgs& a, int num_cells, hipStream_t st, const EamTablePlan& plan)
{
   int want = sim->max_atoms_cell > 0 ? sim->max_atoms_cell + 2 : sim->maxAtoms;
   if (want > sim->maxAtoms) want = sim->maxAtoms;
   int lanes = 4;
   while (lanes < want && lanes < 256) lanes *= 2;
   const int nGroups = ceilDiv(num_cells, 256 / lanes);
   if (plan.spline)                 hipLaunchKernelGGL((EAM_Force_thread_atom<STEP, true, false>), dim3(nGroups), dim3(256), 0, st, a, lanes);
   else if (plan.tablesInLds(STEP)) hipLaunchKernelGGL((EAM_Force_thread_atom<STEP, false, true>), dim3(nGroups < 4096 ? nGroups : 4096), dim3(256), plan.tableBytes(STEP), st, a, lanes);
   else                             hipLaunchKernelGGL((EAM_Force_thread_atom<STEP, false, false>), dim3(nGroups), dim3(256), 0, st, a, lanes);
}

// thread_atom on the brick image (eam_atom_brick_kernels.h)
template <int STEP>
static void launchEamAtomBrick(SimGpu* sim, const EamArgs& a, int num_cells, int* cells_list, hipStream_t st, const EamTablePlan& plan)
{
   const ComdTuning& t = tuningOf(sim);
   const bool tablesInLds = plan.tablesInLds(STEP);
   // a row per thread (bytes: a neighbour is its offset inside its run of the image): the cutoff sphere at the lattice's density + 50 %, a multiple of 8 (an atom
   // with more neighbours walks its stencil a second time); further down it gives up to a fifth of that when the LDS so freed buys a workgroup per CU in pass 1
   int rows = t.eamAtomRows ? t.eamAtomRows : eamRowsPerAtom(sim, 1.5, 32, 128);      // (COMD_EAM_ATOM_ROWS: tests, rows that overflow)
   EamBrickArgs b;
   eamBrickGeometry(sim, &b);      // (the grid; the shape is this method's own)
   const double lat = latticeConstantOf(sim), perCell = 4.0 / (lat * lat * lat) * eamCellVolume(sim);      // atoms of a cell at the lattice's density
   // the threads that take atoms: whole waves for the brick's atoms + 8 % (a fuller brick's threads take a second atom)
   auto rowThreadsOf = [&](double atoms) { int th = ((int)(atoms * 1.08) + 63) / 64 * 64; return th < 64 ? 64 : th > EAM_ATOM_BRICK_THREADS ? EAM_ATOM_BRICK_THREADS : th; };
   // The brick: as many atoms as the workgroup has threads, the block within the 192 cells the staging covers, two workgroups per CU (80 KB of LDS each) in
   // both passes.  Tried in this order; COMD_EAM_ATOM_BRICK="by,bz" overrides.  Fixed by the first launch, the image is sized again when bricks outgrow it.
   const bool handOver = t.eamAtomHandover && rows <= 16 * EAM_ATOM_ROW_CHUNKS;
   if (!sim->eam_pot.atomBrickBy || !sim->eam_pot.atomBrickImageCap) {
      // (larger bricks stage fewer cells per atom and fill six waves -- and are slower: 1 x 5 x 5 1.39 ms, 1 x 4 x 6 1.42, 1 x 5 x 6 1.68 against 1.21 at 80^3; two large
      //  workgroups per CU overlap one's staging with the other's arithmetic less than three small ones)
      static const int shapes[][2] = { { 4, 4 }, { 4, 3 }, { 4, 2 }, { 2, 2 }, { 2, 1 }, { 1, 1 } };
      const bool forced = t.eamAtomBrickBy && 3 * (t.eamAtomBrickBy + 2) * (t.eamAtomBrickBz + 2) <= EAM_ATOM_MAX_CELLS;
      const int nShapes = (int)(sizeof shapes / sizeof shapes[0]);
      for (int k = sim->eam_pot.atomBrickBy ? nShapes - 1 : 0; k < nShapes; ++k) {
         if (sim->eam_pot.atomBrickBy) eamBrickSetShape(&b, sim->eam_pot.atomBrickBy, sim->eam_pot.atomBrickBz);      // (re-sizing: the shape stays)
         else eamBrickSetShape(&b, forced ? t.eamAtomBrickBy : shapes[k][0], forced ? t.eamAtomBrickBz : shapes[k][1]);
         const int cap = eamBrickSizeImage(sim, b, st, false);
         const bool last = forced || sim->eam_pot.atomBrickBy || k == nShapes - 1;
         const int rt = rowThreadsOf(perCell * b.by * b.bz);
         const size_t lds1 = eamAtomBrickLdsBytes(1, plan.tableDoubles(1), cap, rows, rt, true), lds3 = eamAtomBrickLdsBytes(3, plan.tableDoubles(3), cap, rows, rt, !handOver);
         if (last || (perCell * b.by * b.bz <= 1.05 * EAM_ATOM_BRICK_THREADS && lds1 <= 80 * 1024 && lds3 <= 80 * 1024)) {
            sim->eam_pot.atomBrickBy = b.by; sim->eam_pot.atomBrickBz = b.bz; sim->eam_pot.atomBrickImageCap = cap;
            break;
         }
      }
   }
   eamBrickSetShape(&b, sim->eam_pot.atomBrickBy, sim->eam_pot.atomBrickBz);
   b.imageCap = sim->eam_pot.atomBrickImageCap;
   b.listRounds = rowThreadsOf(perCell * b.by * b.bz);      // (EAM_Force_atom_brick reads its row threads here)
   if (!t.eamAtomRows) {
      auto perCu = [&](int r) { return ldsWorkgroupsPerCu(eamAtomBrickLdsBytes(1, plan.tableDoubles(1), b.imageCap, r, b.listRounds, true)); };
      const int least = eamRowsPerAtom(sim, 1.2, 32, 128);
      int best = rows, bestWgs = perCu(rows);
      for (int r = rows - 8; r >= least; r -= 8) if (perCu(r) > bestWgs) { bestWgs = perCu(r); best = r; }
      rows = best;
   }
   b.rows = rows;
   // the rows pass 1 leaves for pass 3 (COMD_EAM_ATOM_HANDOVER=0: pass 3 tests again, A/B runs)
   const int rowCap = b.listRounds <= 192 ? 256 : 512;      // atoms of a brick that can leave a row (a brick fuller than that: its last atoms walk again in pass 3)
   if (handOver && rows <= 16 * EAM_ATOM_ROW_CHUNKS) {
      const size_t nBricks = (size_t)eamBrickCount(b);
      if (!sim->eam_pot.atomRows) {
         sim->eam_pot.atomRows = dalloc<unsigned>(nBricks * EAM_ATOM_ROW_CHUNKS * rowCap * 4, false);
         sim->eam_pot.atomRowCount = dalloc<unsigned short>(nBricks * rowCap * 2, false);      // (a 32-bit word per atom: the three runs' counts)
         sim->eam_pot.atomBrickSel = dalloc<unsigned long long>((size_t)sim->boxes.nLocalBoxes, false);
         HIP_CHECK(hipMemsetAsync(sim->eam_pot.atomBrickSel, 0, (size_t)sim->boxes.nLocalBoxes * sizeof(unsigned long long), st));      // (on the launch stream, like the cell marks)
      }
      if (STEP == 1) sim->eam_pot.atomRowsValid = 1;
      if (STEP == 1 || sim->eam_pot.atomRowsValid) { b.rowsG = sim->eam_pot.atomRows; b.rowCountG = sim->eam_pot.atomRowCount; b.brickSel = sim->eam_pot.atomBrickSel; }
   }
   const int grid = eamBrickCover(sim, &b, num_cells, cells_list, st, false, THREAD_ATOM);
   // pass 3 keeps rows in the LDS only when it has none to read: what they would take is the third workgroup of a CU
   b.listQuads = ((STEP == 3 && b.rowsG) ? 0 : 1) | (rowCap << 8);
   const size_t lds = eamAtomBrickLdsBytes(STEP, plan.tableDoubles(STEP), b.imageCap, b.rows, b.listRounds, (b.listQuads & 1) != 0) + (size_t)t.eamAtomLdsPad;      // (COMD_EAM_ATOM_LDS_PAD: experiments)
   if (lds > 160 * 1024) { fprintf(stderr, "eamForce: thread_atom needs %zu bytes of LDS for this box\n", lds); exit(-1); }
   { ForceLegs& legs = legsOf(sim); legs.eamImage = b.imageCap; legs.eamRows = b.rows; if (STEP == 1) legs.eamPass1Grid = grid; else legs.eamPass3ReadsRows = b.rowsG != nullptr; }
   if (grid <= 0) return;
   // threads: the waves that take atoms, and enough to ask for the 16 first slots of every block cell in EAM_BRICK_STAGE rounds
   const int nThreads = (b.listRounds > 256 || 3 * (b.by + 2) * (b.bz + 2) * 16 > EAM_BRICK_STAGE * 256) ? EAM_ATOM_BRICK_THREADS : 256;
   const bool clampFree = eamClampFree(sim, a, plan.spline);
#define COMD_LAUNCH_EAM_ATOM_BRICK(TAB, SPL, CLP) launchLds(EAM_Force_atom_brick<STEP, TAB, SPL, CLP>, grid, nThreads, lds, st, a, b)
   if (plan.spline)      COMD_LAUNCH_EAM_ATOM_BRICK(false, true, true);
   else if (tablesInLds) { if (clampFree) COMD_LAUNCH_EAM_ATOM_BRICK(true, false, false); else COMD_LAUNCH_EAM_ATOM_BRICK(true, false, true); }
   else                  { if (clampFree) COMD_LAUNCH_EAM_ATOM_BRICK(false, false, false); else COMD_LAUNCH_EAM_ATOM_BRICK(false, false, true); }
#undef COMD_LAUNCH_EAM_ATOM_BRICK
}

// cta_cell and the list method on the brick kernel (eam_brick_kernels.h); STEP 0 is the list build's sweep
template <int STEP>
static void launchEamBrick(SimGpu* sim, const EamArgs& a, int num_cells, int* cells_list, hipStream_t st, const EamTablePlan& plan, bool listed, int method)
{
   EamBrickArgs b;
   eamBrickGeometry(sim, &b); eamBrickOwnShape(sim, listed, &b);
   if (!sim->eam_pot.brickImageCap) sim->eam_pot.brickImageCap = eamBrickSizeImage(sim, b, st, listed);
   b.imageCap = sim->eam_pot.brickImageCap;
   if (listed) {
      NeighborListGpu* n = &sim->atoms.neighborList;
      b.rows = n->brickRowLen; b.rowsG = n->brickRows; b.rowCountG = n->brickRowCount;
      b.listRounds = n->brickRounds; b.listQuads = n->brickQuads;
      const real_t rBuild = sim->eam_pot.cutoff + n->skinDistance;
      b.rBuild2 = rBuild * rBuild;
   } else {
      const int rows = eamRowsPerAtom(sim, 1.5, 32, 256);      // the cutoff sphere + 50 %
      const int lanesMin = (rows + 15) / 16, roundAtoms = 64 / lanesMin < 16 ? 64 / lanesMin : 16;      // (as the kernel derives them from `rows`)
      const int rounds = (sim->maxAtoms + roundAtoms - 1) / roundAtoms;
      if (!sim->eam_pot.pairRows) {                             // rows pass 1 leaves for pass 3: per (cell, round) [2 quads][64 lanes] 16-byte elements
         const size_t slotsLocal = (size_t)sim->boxes.nLocalBoxes * sim->maxAtoms;
         sim->eam_pot.pairRows = dalloc<unsigned>((size_t)sim->boxes.nLocalBoxes * rounds * 2 * 64 * 4, false);
         sim->eam_pot.pairRowCount = dalloc<unsigned short>(slotsLocal, false);      // (written by pass 1 before pass 3 reads it; no zeroing that could race with that)
         sim->eam_pot.pairRowLen = rows;
      }
      b.rows = sim->eam_pot.pairRowLen; b.rowsG = sim->eam_pot.pairRows; b.rowCountG = sim->eam_pot.pairRowCount;
      b.listRounds = rounds; b.listQuads = 2;
      if (!sim->eam_pot.brickSel) {      // (zeroed on the launch stream, like the cell marks)
         sim->eam_pot.brickSel = dalloc<unsigned long long>((size_t)sim->boxes.nLocalBoxes, false);
         HIP_CHECK(hipMemsetAsync(sim->eam_pot.brickSel, 0, (size_t)sim->boxes.nLocalBoxes * sizeof(unsigned long long), st));
      }
      b.brickSel = sim->eam_pot.brickSel;
   }
   const int grid = eamBrickCover(sim, &b, num_cells, cells_list, st, listed, method);
   const int waves = 4;     // EAM_Force_cta_brick is written for 256 threads: __launch_bounds__(256, 4), staging loops of STAGE x 256 tasks
   if (listed && 3 * (b.by + 2) * (b.bz + 2) * 32 > EAM_BRICK_STAGE_LISTED * 64 * waves) { fprintf(stderr, "eamForce: a brick of 1 x %d x %d cells has more cells around it than a listed launch stages\n", b.by, b.bz); exit(-1); }
   const size_t lds = eamBrickLdsBytes(STEP, listed, plan.tableDoubles(STEP), b.imageCap, b.rows, waves);
   if (lds > 160 * 1024) { fprintf(stderr, "eamForce: cta_cell needs %zu bytes of LDS for this box\n", lds); exit(-1); }
   { ForceLegs& legs = legsOf(sim); legs.eamImage = b.imageCap; legs.eamRows = b.rows; if (STEP != 3) legs.eamPass1Grid = grid; else legs.eamPass3ReadsRows = 1; }
   if (grid <= 0) return;
   const bool tablesInLds = plan.tablesInLds(STEP), clampFree = eamClampFree(sim, a, plan.spline);
#define COMD_LAUNCH_EAM_BRICK(STP, TAB, SPL, LST, CLP) launchLds(EAM_Force_cta_brick<STP, TAB, SPL, LST, CLP>, grid, 64 * waves, lds, st, a, b)
#define COMD_LAUNCH_EAM_BRICK_C(STP, TAB, LST) do { if (clampFree) COMD_LAUNCH_EAM_BRICK(STP, TAB, false, LST, false); else COMD_LAUNCH_EAM_BRICK(STP, TAB, false, LST, true); } while (0)
   if (STEP == 0)        COMD_LAUNCH_EAM_BRICK(0, false, false, true, true);
   else if (listed) {
      if (plan.spline)      COMD_LAUNCH_EAM_BRICK((STEP == 0 ? 1 : STEP), false, true, true, true);
      else if (tablesInLds) COMD_LAUNCH_EAM_BRICK_C((STEP == 0 ? 1 : STEP), true, true);
      else                  COMD_LAUNCH_EAM_BRICK_C((STEP == 0 ? 1 : STEP), false, true);
   } else {
      if (plan.spline)      COMD_LAUNCH_EAM_BRICK((STEP == 0 ? 1 : STEP), false, true, false, true);
      else if (tablesInLds) COMD_LAUNCH_EAM_BRICK_C((STEP == 0 ? 1 : STEP), true, false);
      else                  COMD_LAUNCH_EAM_BRICK_C((STEP == 0 ? 1 : STEP), false, false);
   }
#undef COMD_LAUNCH_EAM_BRICK_C
#undef COMD_LAUNCH_EAM_BRICK
}
// COMD_EAM_NL=lds: round 3's list kernel, 16-bit entries into a wave's staging of the whole 27-cell stencil (nl_kernels.h EAM_Force_nl_lds)
template <int STEP>
static void launchEamNlLds(SimGpu* sim, const EamArgs& a, int num_cells, hipStream_t st, const EamTablePlan& plan)
{
   NeighborListGpu* n = &sim->atoms.neighborList;
   (void)nlView(sim);
   NlSlabView v; v.list = n->list16; v.count = n->nNeighbors; v.rows = n->slabRows;
   const size_t lds = eamNlLdsBytes(STEP, a.rho.n, a.phi.n, plan.sameGrid, n->maxSlabAtoms, plan.spline);
   if (lds > 160 * 1024) { fprintf(stderr, "eamForce: %d atoms in a 27-cell stencil do not fit the LDS\n", n->maxSlabAtoms); exit(-1); }
   const int grid = ceilDiv(num_cells, EAM_NL_WAVES * 8);        // each wave walks ~8 consecutive cells
   if (plan.spline) launchLds(EAM_Force_nl_lds<STEP, true>, grid, 64 * EAM_NL_WAVES, lds, st, a, v, n->maxSlabAtoms);
   else             launchLds(EAM_Force_nl_lds<STEP, false>, grid, 64 * EAM_NL_WAVES, lds, st, a, v, n->maxSlabAtoms);
}
// COMD_NL_GLOBAL=1: lists of global slots
template <int STEP>
static void launchEamThreadAtomNl(SimGpu* sim, const EamArgs& a, int num_cells, hipStream_t st, const EamTablePlan& plan)
{
   const NlView nl = nlView(sim);
   const unsigned nBlocks = (unsigned)ceilDiv((long)num_cells * sim->maxAtoms, 256);
   if (plan.spline)                 hipLaunchKernelGGL((EAM_Force_thread_atom_nl<STEP, false, true>), dim3(nBlocks), dim3(256), 0, st, a, nl);
   else if (plan.tablesInLds(STEP)) hipLaunchKernelGGL((EAM_Force_thread_atom_nl<STEP, true, false>), dim3(nBlocks), dim3(256), plan.tableBytes(STEP), st, a, nl);
   else                             hipLaunchKernelGGL((EAM_Force_thread_atom_nl<STEP, false, false>), dim3(nBlocks), dim3(256), 0, st, a, nl);
}
// COMD_EAM_CTA=cell: round 2's form, a wave stages the stencil of every cell for itself (nl_kernels.h EAM_Force_cta_cell); kept for A/B runs
template <int STEP>
static void launchEamCtaCell(SimGpu* sim, const EamArgs& a, int num_cells, hipStream_t st, const EamTablePlan& plan)
{
   const ComdTuning& t = tuningOf(sim);
   // a stencil of 27 cells at the perfect-lattice density + 30 % (thermal crowding, cells fuller than the mean), whole staging rounds of 64
   const double lat = latticeConstantOf(sim), perStencil = 27.0 * eamCellVolume(sim) * 4.0 / (lat * lat * lat);
   int stencil = (((int)(perStencil * 1.30) + 16 + 7) / 8) * 8;
   if (stencil < 128) stencil = 128;
   if (stencil > 27 * sim->maxAtoms) stencil = ((27 * sim->maxAtoms + 7) / 8) * 8;
   if (stencil > 1024) stencil = 1024;                    // beyond that a cell takes the thread-per-atom form inside the same kernel
   // rows per atom: the cutoff sphere + 50 %; the hand-over holds 16 lanes x 8 trips x 2 numbers per atom
   const int rows = eamRowsPerAtom(sim, 1.5, 32, 256);
   // 4 waves per workgroup, one per SIMD (5 or 6 land unevenly on the four SIMDs of a CU: measured 3.4-3.7 ms against 2.6 at 80^3)
   const int waves = t.eamCtaWaves ? t.eamCtaWaves : 4;
   if (!sim->eam_pot.pairRows) {                          // first cta_cell launch: rows pass 1 leaves for pass 3
      const size_t slotsLocal = (size_t)sim->boxes.nLocalBoxes * sim->maxAtoms;
      sim->eam_pot.pairRows = dalloc<unsigned>(slotsLocal * EAM_ROW_WORDS, false);
      sim->eam_pot.pairRowCount = dalloc<unsigned short>(slotsLocal, false);
      sim->eam_pot.pairRowLen = rows;
   }
   // The LDS slice decides how many workgroups share a CU, and these kernels live on latency hiding: at 80^3 a slice of 384 records leaves room for two
   // workgroups per CU in either pass, one of 376 for three (measured: pass 1 1.43 -> 1.08 ms).  Shrink the slice, down to the density + 20 %, when that
   // buys a workgroup in pass 1 or pass 3; both passes must use the same size (a cell either has rows or takes the thread-per-atom form, in both).
   auto ldsBytes = [&](int step, int records) { return eamCtaCellLdsBytes(step, a.rho.n, a.phi.n, plan.tablesInLds(step), plan.sameGrid, records, rows, waves); };
   auto perCu = [&](int records) { return ldsWorkgroupsPerCu(ldsBytes(1, records)) + ldsWorkgroupsPerCu(ldsBytes(3, records)); };
   const int lo = (((int)(perStencil * 1.20) + 16 + 7) / 8) * 8;
   int best = stencil, bestScore = perCu(stencil);
   for (int s = stencil - 8; s >= lo && s >= 128; s -= 8) if (perCu(s) > bestScore) { bestScore = perCu(s); best = s; }
   stencil = t.eamStencil ? t.eamStencil : best;          // (COMD_EAM_STENCIL, experiments: LDS slice size)
   const size_t lds = ldsBytes(STEP, stencil);
   if (lds > 160 * 1024) { fprintf(stderr, "eamForce: cta_cell needs %zu bytes of LDS for this box\n", lds); exit(-1); }
   const int grid = ceilDiv(num_cells, waves * 8);        // each wave walks ~8 consecutive cells
   { ForceLegs& legs = legsOf(sim); legs.eamStencil = stencil; legs.eamRows = rows; if (STEP == 3) legs.eamPass3ReadsRows = 1; }
#define COMD_LAUNCH_EAM_CTA(TAB, SPL) launchLds(EAM_Force_cta_cell<STEP, TAB, SPL>, grid, 64 * waves, lds, st, a, stencil, rows, sim->eam_pot.pairRows, sim->eam_pot.pairRowCount, sim->fuseEmbed, sim->status)
   if (plan.spline)                 COMD_LAUNCH_EAM_CTA(false, true);
   else if (plan.tablesInLds(STEP)) COMD_LAUNCH_EAM_CTA(true, false);
   else                             COMD_LAUNCH_EAM_CTA(false, false);
#undef COMD_LAUNCH_EAM_CTA
}

// One pair pass (1: densities, 3: forces) of a force evaluation over `cells_list`: the path predicates above decide the kernel
template <int STEP>
static void launchEamPair(SimGpu* sim, int num_cells, int* cells_list, int method, hipStream_t st, int spline)
{
   if (num_cells <= 0) return;
   EamArgs a = makeEamArgs(sim, num_cells, cells_list);
   const EamTablePlan plan(a.phi, a.rho, spline);
   ForceTimer timer(sim, st);
   // -P (gpu_kernels.cu:164-226): cubic splines in r^2 for phi and rho, coefficient tables read through L2 (16 KB each for funcfl)
   if (spline && (!a.phiS.coefficients || !a.rhoS.coefficients)) { fprintf(stderr, "eamForce: spline != 0 but no spline tables were given to AllocateGpu\n"); exit(-1); }
   const bool lists = method == THREAD_ATOM_NL || method == WARP_ATOM_NL, atomBrick = eamAtomBrickPath(sim, method);
   if (STEP == 1 && !atomBrick) sim->eam_pot.atomRowsValid = 0;      // (another method's pass 1: the rows EAM_Force_atom_brick left are not this evaluation's)
   // what this launch runs, for comdForceLegReport (the brick launchers add their shape, image and rows)
   ForceLegs& legs = legsOf(sim);
   legs.eamCover = cells_list ? 2 : 0; legs.eamSpline = plan.spline; legs.eamClampsKept = !eamClampFree(sim, a, plan.spline);
   if (STEP == 1) { legs.eamTablesInLds = plan.tablesInLds(1); legs.eamPass3ReadsRows = 0; legs.eamBy = legs.eamBz = legs.eamImage = legs.eamBricks = legs.eamPass1Grid = legs.eamRows = legs.eamStencil = 0; legs.eamRunMax = 0; }
   if (!lists && method != CTA_CELL && !atomBrick) { legs.eamKernel = 6; launchEamThreadAtom<STEP>(sim, a, num_cells, st, plan); }
   else if (atomBrick)                             { legs.eamKernel = 2; launchEamAtomBrick<STEP>(sim, a, num_cells, cells_list, st, plan); }
   else if (eamListedBrick(sim, method)) {
      if (sim->atoms.neighborList.nBuilds == 0) { fprintf(stderr, "the *_nl methods need buildNeighborListGpu before the first force call\n"); exit(-1); }
      legs.eamKernel = 4; launchEamBrick<STEP>(sim, a, num_cells, cells_list, st, plan, true, method);
   }
   else if (lists && sim->atoms.neighborList.slabFormat == 2) { legs.eamKernel = 5; launchEamNlLds<STEP>(sim, a, num_cells, st, plan); }
   else if (lists)                                 { legs.eamKernel = 7; launchEamThreadAtomNl<STEP>(sim, a, num_cells, st, plan); }
   else if (eamBrickPath(sim, method))             { legs.eamKernel = 1; launchEamBrick<STEP>(sim, a, num_cells, cells_list, st, plan, false, method); }
   else                                            { legs.eamKernel = 3; launchEamCtaCell<STEP>(sim, a, num_cells, st, plan); }
   LAUNCH_CHECK();
}

// cta_cell: size the brick image again at the next launch (between two force evaluations only: pass 1 and pass 3 of one evaluation must stage alike)
extern "C" void comdEamBrickResize(SimGpu* sim) { sim->eam_pot.brickImageCap = 0; sim->eam_pot.atomBrickImageCap = 0; }
extern "C" void comdEamBrickStats(SimGpu* sim, int out[3])
{
   out[0] = out[1] = out[2] = 0;
   if (!sim->eam_pot.brickStats) return;
   int h[2];
   HIP_CHECK(hipDeviceSynchronize());
   HIP_CHECK(hipMemcpy(h, sim->eam_pot.brickStats, sizeof h, hipMemcpyDeviceToHost));
   HIP_CHECK(hipMemset(sim->eam_pot.brickStats + 1, 0, sizeof(int)));
   const bool atomBrick = !sim->eam_pot.brickBy && sim->eam_pot.atomBrickBy;      // (thread_atom on the brick image: its shape, its image)
   int by = atomBrick ? sim->eam_pot.atomBrickBy : sim->eam_pot.brickBy ? sim->eam_pot.brickBy : 4, bz = atomBrick ? sim->eam_pot.atomBrickBz : sim->eam_pot.brickBz ? sim->eam_pot.brickBz : 2;
   out[0] = h[1]; out[1] = sim->boxes.gridSize[0] * ceilDiv(sim->boxes.gridSize[1], by) * ceilDiv(sim->boxes.gridSize[2], bz);
   out[2] = atomBrick ? sim->eam_pot.atomBrickImageCap : sim->eam_pot.brickImageCap;
}
extern "C" void eamForce1GpuAsync(SimGpu* sim, int num_cells, int* cells_list, int method, comdStream_t stream, int spline) { launchEamPair<1>(sim, num_cells, cells_list, method, S(stream), spline); }
extern "C" void eamForce3GpuAsync(SimGpu* sim, int num_cells, int* cells_list, int method, comdStream_t stream, int spline) { launchEamPair<3>(sim, num_cells, cells_list, method, S(stream), spline); }
extern "C" void eamForce2GpuAsync(SimGpu* sim, int num_cells, int* cells_list, int method, comdStream_t stream, int spline)
{
   (void)spline;                            /* F(rhobar) is quadratic in both modes (gpu_utility.c:443) */
   if (num_cells <= 0) return;
   if (sim->fuseEmbed && (method == CTA_CELL || eamListedBrick(sim, method) || eamAtomBrickPath(sim, method))) return;      /* eamForce1Gpu[Async] has done it for these cells (SimGpu.fuseEmbed) */
   EamArgs a = makeEamArgs(sim, num_cells, cells_list);
   // cta_cell in the overlap mode: pass 1 took whole bricks (launchEamBrick), the embedding follows the same groups over all local cells
   const int group = sim->eam_pot.brickGroup ? eamBrickGroupOf(sim, cells_list, num_cells, method) : 0;
   if (group) { a.cells = nullptr; a.nCells = num_cells = sim->boxes.nLocalBoxes; a.sel = sim->eam_pot.brickGroup; a.tag = group; }
   ForceTimer timer(sim, S(stream));
   hipLaunchKernelGGL(EAM_Force_embed, dim3(ceilDiv((long)num_cells * sim->maxAtoms, 256)), dim3(256), 0, S(stream), a);
   LAUNCH_CHECK();
}
extern "C" void eamForce1Gpu(SimGpu* sim, int method, int spline) { eamForce1GpuAsync(sim, sim->boxes.nLocalBoxes, nullptr, method, nullptr, spline); }
extern "C" void eamForce2Gpu(SimGpu* sim, int method, int spline) { eamForce2GpuAsync(sim, sim->boxes.nLocalBoxes, nullptr, method, nullptr, spline); }
extern "C" void eamForce3Gpu(SimGpu* sim, int method, int spline) { eamForce3GpuAsync(sim, sim->boxes.nLocalBoxes, nullptr, method, nullptr, spline); }
