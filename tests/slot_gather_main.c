/* slot_gather_main.c -- TEST INFRASTRUCTURE: slotGather (csrc/host/slot_gather.h) on the smallest arrays that can go wrong, built with
 * -fsanitize=address,undefined by tests/test_slot_gather.py, in both precisions.
 *
 * 3 cells of capacity 4 with occupancies {0, 4, 2}; 8 global ids; the occupied slots hold the gids 5, 0, 8 (out of range: skipped), 3 | 7, 2, so the gids
 * 1, 4 and 6 are absent.  The by-slot arrays end with the last occupied slot of the last cell: a read of one of its unoccupied slots runs past the
 * allocation.  The unoccupied slots inside the arrays (cell 0) hold NaN / -1 and the gid 1.  The destinations hold exactly the 8 gids: a write for gid 8
 * runs past them. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "slot_gather.h"

#define CELLS 3
#define CAP 4
#define N 8
#define EXTENT (2 * CAP + 2)      /* slots up to the last occupied one */

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "slot_gather_main: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(void)
{
   const int nAtoms[CELLS] = { 0, 4, 2 };
   const int gidOf[EXTENT] = { 1, 1, 1, 1, 5, 0, 8, 3, 7, 2 };
   int* gid = (int*)malloc(EXTENT * sizeof(int));
   real_t* a = (real_t*)malloc(EXTENT * sizeof(real_t));
   real_t* b = (real_t*)malloc(EXTENT * sizeof(real_t));
   int* c = (int*)malloc(EXTENT * sizeof(int));
   for (int o = 0; o < EXTENT; ++o) {
      const int occupied = o >= CAP;
      gid[o] = gidOf[o];
      a[o] = occupied ? (real_t)(o + 0.5) : (real_t)NAN;
      b[o] = occupied ? (real_t)(-2.0 * o - 0.25) : (real_t)NAN;
      c[o] = occupied ? 100 + o : -1;
   }
   double* ab = (double*)malloc(N * 2 * sizeof(double));      /* [N][2] */
   int* cc = (int*)malloc(N * sizeof(int));
   for (int g = 0; g < N; ++g) { ab[2 * g] = ab[2 * g + 1] = 77.0; cc[g] = 77; }      /* slotGather zeroes them */

   const SlotPlane planes[3] = { { a, SLOT_REAL, ab, 2, 0 }, { b, SLOT_REAL, ab, 2, 1 }, { c, SLOT_INT, cc, 1, 0 } };
   slotGather(nAtoms, gid, CELLS, CAP, N, planes, 3);

   int slotOf[N];
   for (int g = 0; g < N; ++g) slotOf[g] = -1;
   for (int o = CAP; o < EXTENT; ++o) if (gidOf[o] < N) slotOf[gidOf[o]] = o;
   int present = 0;
   for (int g = 0; g < N; ++g) {
      const int o = slotOf[g];
      CHECK(!isnan(ab[2 * g]) && !isnan(ab[2 * g + 1]) && cc[g] != -1);
      if (o < 0) { CHECK(ab[2 * g] == 0.0 && ab[2 * g + 1] == 0.0 && cc[g] == 0); continue; }
      present++;
      CHECK(ab[2 * g] == (double)(real_t)(o + 0.5) && ab[2 * g + 1] == (double)(real_t)(-2.0 * o - 0.25) && cc[g] == 100 + o);
   }
   CHECK(present == 5);

   /* a count plane into doubles, as the coordination of comdCentroSymmetry */
   const SlotPlane asDouble = { c, SLOT_INT_AS_DOUBLE, ab, 2, 1 };
   slotGather(nAtoms, gid, CELLS, CAP, N, &asDouble, 1);
   for (int g = 0; g < N; ++g) CHECK(ab[2 * g + 1] == (slotOf[g] < 0 ? 0.0 : 100.0 + slotOf[g]));

   free(gid); free(a); free(b); free(c); free(ab); free(cc);
   printf("slot_gather_main OK\n");
   return 0;
}
