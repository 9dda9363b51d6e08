/* slot_gather.h -- by-slot results of the local cells into by-gid arrays: the pass of the by-gid analyses (analysis.c).  A pure function of host arrays, so
 * that it can be compiled and run on its own (tests/slot_gather_main.c). */
#ifndef SLOT_GATHER_H
#define SLOT_GATHER_H
#include <stddef.h>
#include <string.h>
#include "comd_hip.h"      /* real_t */

enum { SLOT_REAL, SLOT_INT, SLOT_INT_AS_DOUBLE };      /* a plane of real_t into doubles, of int into ints, of int into doubles */

/* one by-slot plane [nLocalBoxes * cap] and where its value of the atom gid goes: dst[stride * gid + offset] */
typedef struct {
   const void* src;
   int kind;
   void* dst;
   size_t stride, offset;
} SlotPlane;

/* `len` planes of one kind that follow one another in the rows of one destination: zero the rows (a memset when the run is the whole row), then one tight
 * loop over the planes per occupied slot */
#define SLOT_GATHER_RUN(SRC, DST) do { \
   DST* d = (DST*)p->dst + p->offset; \
   if ((size_t)len == stride && p->offset == 0) memset(d, 0, n * stride * sizeof(DST)); \
   else for (size_t g = 0; g < n; ++g) for (int c = 0; c < len; ++c) d[stride * g + c] = 0; \
   for (int b = 0; b < nLocalBoxes; ++b) \
      for (size_t o = (size_t)b * cap, e = o + (size_t)nAtoms[b]; o < e; ++o) { \
         const size_t g = (size_t)gid[o]; \
         if (g < n) for (int c = 0; c < len; ++c) d[stride * g + c] = (DST)((const SRC*)p[c].src)[o]; \
      } \
} while (0)

/* The destinations of the gids 0 .. n-1 are zeroed, then every occupied slot (cell b holds nAtoms[b] atoms in its first slots, gid[] by slot) writes the
 * destinations of its gid.  A gid outside [0, n) is skipped; no plane and no gid is read at or beyond a cell's occupancy. */
static inline void slotGather(const int* nAtoms, const int* gid, int nLocalBoxes, int cap, size_t n, const SlotPlane* planes, int nPlanes)
{
   for (int k = 0, len; k < nPlanes; k += len) {
      const SlotPlane* p = planes + k;
      const size_t stride = p->stride;
      for (len = 1; k + len < nPlanes && p[len].kind == p->kind && p[len].dst == p->dst && p[len].stride == stride && p[len].offset == p->offset + len; ++len) ;
      if (p->kind == SLOT_REAL) SLOT_GATHER_RUN(real_t, double);
      else if (p->kind == SLOT_INT) SLOT_GATHER_RUN(int, int);
      else SLOT_GATHER_RUN(int, double);
   }
}
#endif
