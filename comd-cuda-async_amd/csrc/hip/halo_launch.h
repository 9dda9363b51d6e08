// halo_launch.h -- the halo launch layer: pack, unpack, mirror and scan of the cells an exchange names, and the blocking and mirrored reads of its message counts.
// Host code, part of comd_device.hip's translation unit (it uses HIP_CHECK, LAUNCH_CHECK, S, ceilDiv, atomArrays, sortBlock and comdReadDeviceInt of that file).  Every
// entry takes both faces of an axis phase; the one-face entries with the reference's names are these with one face.  The offsets of a dF/drho or position message are
// the caller's to scan (scanCellListsGpu) before it packs or unpacks: only the one-face entries of the reference-side adapter scan their own list.
#pragma once

extern "C" void getAtomMsgSoAPtr(char* buffer, AtomMsgSoA* m, int n)
{
   m->gid = (int*)(buffer + COMD_ATOM_MSG_HEADER);
   m->type = m->gid + n;
   m->rx = (real_t*)(m->type + n);
   m->ry = m->rx + n; m->rz = m->ry + n; m->px = m->rz + n; m->py = m->px + n; m->pz = m->py + n;
}

static int maxInt(int a, int b) { return a > b ? a : b; }

// both faces of an axis phase: one scan launch (two jobs), one pack launch (blockIdx.y = face)
extern "C" void compactCellsGpu2(char* workM, char* workP, const int nCells[2], int* const d_cellList[2], SimGpu* sim, int* const d_cellOffsets[2],
                                 const real_t shiftM[3], const real_t shiftP[3], const int capacityAtoms[2], comdStream_t stream)
{
   hipStream_t st = S(stream);
   const int nFaces = workP ? 2 : 1;
   ScanJobs jobs;
   AtomPackJob pj[2];
   char* work[2] = { workM, workP };
   const real_t* shift[2] = { shiftM, shiftP };
   for (int f = 0; f < 2; ++f) {
      const int k = f < nFaces ? f : 0;
      jobs.list[f] = d_cellList[k]; jobs.n[f] = nCells[k]; jobs.out[f] = d_cellOffsets[k]; jobs.total[f] = (int*)work[k];
      pj[f].msg = work[k]; pj[f].list = d_cellList[k]; pj[f].offsets = d_cellOffsets[k]; pj[f].nCells = nCells[k];
      pj[f].sx = shift[k][0]; pj[f].sy = shift[k][1]; pj[f].sz = shift[k][2]; pj[f].capacityAtoms = capacityAtoms[k];
   }
   hipLaunchKernelGGL(ScanCellCountsBatch, dim3(nFaces), dim3(1024), 0, st, sim->boxes.nAtoms, jobs);
   hipLaunchKernelGGL(LoadAtomsBufferPacked, dim3(nFaces == 2 ? maxInt(nCells[0], nCells[1]) : nCells[0], nFaces), dim3(sortBlock(sim->maxAtoms)), 0, st,
                      pj[0], pj[1], atomArrays(sim), sim->boxes.nAtoms, sim->maxAtoms, sim->status);
   LAUNCH_CHECK();
}

extern "C" void compactCellsGpu(char* work_d, int nCells, int* d_cellList, SimGpu* sim, int* d_cellOffsets,
                                const real_t shift[3], int capacityAtoms, comdStream_t stream)
{
   const int n[2] = { nCells, 0 }; int* const lists[2] = { d_cellList, nullptr }; int* const offs[2] = { d_cellOffsets, nullptr };
   const int caps[2] = { capacityAtoms, 0 };
   compactCellsGpu2(work_d, nullptr, n, lists, sim, offs, shift, shift, caps, stream);
}

extern "C" void comdReadDeviceInt2(const int* d_a, const int* d_b, int out[2], comdStream_t stream)
{
   HIP_CHECK(hipMemcpyAsync(&out[0], d_a, sizeof(int), hipMemcpyDeviceToHost, S(stream)));
   HIP_CHECK(hipMemcpyAsync(&out[1], d_b, sizeof(int), hipMemcpyDeviceToHost, S(stream)));
   HIP_CHECK(hipStreamSynchronize(S(stream)));
}

extern "C" void comdMirrorCounts(const int* d0, const int* d1, const int* d2, const int* d3, int* pinnedDst, comdStream_t stream)
{
   hipLaunchKernelGGL(MirrorCounts, dim3(1), dim3(64), 0, S(stream), d0, d1, d2, d3, pinnedDst);
   LAUNCH_CHECK();
}

extern "C" int atomMsgCountGpu(SimGpu* sim, const char* msg_d, comdStream_t stream)
{
   (void)sim;
   return comdReadDeviceInt((const int*)msg_d, stream);
}

// msgB == NULL: one message
extern "C" void unloadAtomsBufferToGpu2(const char* msgA, int nBufA, int maxAtomsA, const char* msgB, int nBufB, int maxAtomsB, SimGpu* sim, comdStream_t stream)
{
   const int boundA = nBufA >= 0 ? nBufA : maxAtomsA, boundB = msgB ? (nBufB >= 0 ? nBufB : maxAtomsB) : 0;
   const int bound = maxInt(boundA, boundB);
   if (bound <= 0) return;
   AtomUnpackJob a = { msgA, nBufA, maxAtomsA }, b = { msgB ? msgB : msgA, msgB ? nBufB : 0, msgB ? maxAtomsB : 0 };
   hipLaunchKernelGGL(UnloadAtomsBufferPacked, dim3(ceilDiv(bound, 256), msgB ? 2 : 1), dim3(256), 0, S(stream), a, b,
                      atomArrays(sim), sim->boxes.nAtoms, sim->cellDirty, sim->status, sim->boxes, sim->maxAtoms);
   LAUNCH_CHECK();
}

extern "C" void unloadAtomsBufferToGpu(const char* msg_d, int nBuf, int maxAtomsInMsg, SimGpu* sim, comdStream_t stream)
{
   unloadAtomsBufferToGpu2(msg_d, nBuf, maxAtomsInMsg, nullptr, 0, 0, sim, stream);
}

extern "C" void scanCellListsGpu(SimGpu* sim, int nLists, int** d_cellLists, const int* nCells, int** d_cellOffsets, comdStream_t stream)
{
   if (nLists < 1 || nLists > 12) { fprintf(stderr, "scanCellListsGpu: 1..12 lists per call\n"); exit(-1); }
   ScanJobs jobs;
   for (int i = 0; i < 12; ++i) { const int k = i < nLists ? i : 0; jobs.list[i] = d_cellLists[k]; jobs.n[i] = nCells[k]; jobs.out[i] = d_cellOffsets[k]; jobs.total[i] = nullptr; }
   hipLaunchKernelGGL(ScanCellCountsBatch, dim3(nLists), dim3(1024), 0, S(stream), sim->boxes.nAtoms, jobs);
   LAUNCH_CHECK();
}

static SlotJob slotJob(const real_t* buf, int nCells, int* list, int* offsets, int bound, const real_t* shift)
{
   SlotJob j; j.buf = (real_t*)buf; j.list = list; j.offsets = offsets; j.nCells = nCells; j.boundAtoms = bound;
   j.sx = shift ? shift[0] : 0.0; j.sy = shift ? shift[1] : 0.0; j.sz = shift ? shift[2] : 0.0;
   return j;
}

// kind 0: dF/drho (1 real per atom), 1: positions + shift (3 reals per atom); bufP == NULL: one face.  offsets[] hold the scan of the listed cells' occupancies
// (scanCellListsGpu: dF/drho once the atom exchange of the step has been sorted, positions after the list build whose slots they keep)
static void loadSlotBuffers(int kind, real_t* bufM, real_t* bufP, const int nCells[2], int* const lists[2], int* const offsets[2], const int bounds[2],
                            const real_t* shiftM, const real_t* shiftP, SimGpu* sim, hipStream_t st)
{
   const int nFaces = bufP ? 2 : 1;
   const SlotJob a = slotJob(bufM, nCells[0], lists[0], offsets[0], bounds[0], shiftM);
   const SlotJob b = bufP ? slotJob(bufP, nCells[1], lists[1], offsets[1], bounds[1], shiftP) : a;
   const dim3 grid(nFaces == 2 ? maxInt(nCells[0], nCells[1]) : nCells[0], nFaces), block(sortBlock(sim->maxAtoms));
   if (kind == 0) hipLaunchKernelGGL(LoadForceBuffer, grid, block, 0, st, a, b, sim->eam_pot.dfEmbed, sim->boxes.nAtoms, sim->maxAtoms, sim->status);
   else           hipLaunchKernelGGL(LoadPositionBuffer, grid, block, 0, st, a, b, sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->boxes.nAtoms, sim->maxAtoms, sim->status);
   LAUNCH_CHECK();
}

static void unloadSlotBuffers(int kind, const real_t* bufA, const real_t* bufB, const int nCells[2], int* const lists[2], int* const offsets[2],
                              SimGpu* sim, hipStream_t st)
{
   const int nFaces = bufB ? 2 : 1;
   const SlotJob a = slotJob(bufA, nCells[0], lists[0], offsets[0], 0, nullptr);
   const SlotJob b = bufB ? slotJob(bufB, nCells[1], lists[1], offsets[1], 0, nullptr) : a;
   const dim3 grid(nFaces == 2 ? maxInt(nCells[0], nCells[1]) : nCells[0], nFaces), block(sortBlock(sim->maxAtoms));
   if (kind == 0) hipLaunchKernelGGL(UnloadForceBuffer, grid, block, 0, st, a, b, sim->eam_pot.dfEmbed, sim->boxes.nAtoms, sim->maxAtoms);
   else           hipLaunchKernelGGL(UnloadPositionBuffer, grid, block, 0, st, a, b, sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->boxes.nAtoms, sim->maxAtoms);
   LAUNCH_CHECK();
}

// the reference's one-face entries (include/comd_hip_shim.h): each scans its own list first, no agreed size (bound 0)
extern "C" void loadForceBufferFromGpu(real_t* gpu_buf, int nCells, int* d_cellList, int* d_cellOffsets, SimGpu* sim, comdStream_t stream)
{
   const int n[2] = { nCells, 0 }; int* const l[2] = { d_cellList, nullptr }; int* const o[2] = { d_cellOffsets, nullptr }; const int b[2] = { 0, 0 };
   scanCellListsGpu(sim, 1, &d_cellList, &nCells, &d_cellOffsets, stream);
   loadSlotBuffers(0, gpu_buf, nullptr, n, l, o, b, nullptr, nullptr, sim, S(stream));
}

extern "C" void unloadForceBufferToGpu(const real_t* gpu_buf, int nCells, int* d_cellList, int* d_cellOffsets, SimGpu* sim, comdStream_t stream)
{
   const int n[2] = { nCells, 0 }; int* const l[2] = { d_cellList, nullptr }; int* const o[2] = { d_cellOffsets, nullptr };
   scanCellListsGpu(sim, 1, &d_cellList, &nCells, &d_cellOffsets, stream);
   unloadSlotBuffers(0, gpu_buf, nullptr, n, l, o, sim, S(stream));
}

extern "C" void loadForceBufferFromGpu2(real_t* bufM, real_t* bufP, const int nCells[2], int* const d_cellList[2], int* const d_cellOffsets[2],
                                        const int boundAtoms[2], SimGpu* sim, comdStream_t stream)
{ loadSlotBuffers(0, bufM, bufP, nCells, d_cellList, d_cellOffsets, boundAtoms, nullptr, nullptr, sim, S(stream)); }

extern "C" void unloadForceBufferToGpu2(const real_t* bufA, const real_t* bufB, const int nCells[2], int* const d_cellList[2], int* const d_cellOffsets[2],
                                        SimGpu* sim, comdStream_t stream)
{ unloadSlotBuffers(0, bufA, bufB, nCells, d_cellList, d_cellOffsets, sim, S(stream)); }

extern "C" void loadPositionBufferFromGpu2(real_t* bufM, real_t* bufP, const int nCells[2], int* const d_cellList[2], int* const d_cellOffsets[2],
                                           const int boundAtoms[2], const real_t shiftM[3], const real_t shiftP[3], SimGpu* sim, comdStream_t stream)
{ loadSlotBuffers(1, bufM, bufP, nCells, d_cellList, d_cellOffsets, boundAtoms, shiftM, shiftP, sim, S(stream)); }

extern "C" void unloadPositionBufferToGpu2(const real_t* bufA, const real_t* bufB, const int nCells[2], int* const d_cellList[2], int* const d_cellOffsets[2],
                                           SimGpu* sim, comdStream_t stream)
{ unloadSlotBuffers(1, bufA, bufB, nCells, d_cellList, d_cellOffsets, sim, S(stream)); }

extern "C" void mirrorAtomCellsGpu(const int nCells[2], int* const d_cellList[2], const real_t shiftM[3], const real_t shiftP[3], int firstAxis, int axis,
                                   SimGpu* sim, comdStream_t stream)
{
   MirrorAtomsJob jb;
   for (int f = 0; f < 2; ++f) {
      const real_t* sh = f ? shiftP : shiftM;
      jb.list[f] = d_cellList[f]; jb.nCells[f] = nCells[f]; jb.sx[f] = sh[0]; jb.sy[f] = sh[1]; jb.sz[f] = sh[2];
   }
   const int most = maxInt(nCells[0], nCells[1]);
   if (most <= 0) return;
   hipLaunchKernelGGL(MirrorAtomCells, dim3(ceilDiv((long)most * sim->maxAtoms, 256), 2), dim3(256), 0, S(stream), jb, atomArrays(sim), sim->boxes.nAtoms,
                      sim->cellArrivals, sim->boxes.nTotalBoxes, firstAxis, axis, sim->cellDirty, sim->status, sim->boxes, sim->maxAtoms);
   LAUNCH_CHECK();
}

extern "C" void mirrorSlotCellsGpu(int kind, int nPairs, const int* d_dst, const int* d_src, const real_t* d_shift, SimGpu* sim, comdStream_t stream)
{
   if (nPairs <= 0) return;
   hipLaunchKernelGGL(MirrorSlotCells, dim3(nPairs), dim3(sortBlock(sim->maxAtoms)), 0, S(stream), kind, nPairs, d_dst, d_src, d_shift,
                      sim->atoms.r.x, sim->atoms.r.y, sim->atoms.r.z, sim->eam_pot.dfEmbed, sim->boxes.nAtoms, sim->maxAtoms);
   LAUNCH_CHECK();
}
