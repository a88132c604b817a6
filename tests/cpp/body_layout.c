/* Prints sizeof / offsetof of the body records of include/dust_hip.h and the call's constants, one "name value" per line
   (tests/test_body_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipBodyQuery %zu\n", sizeof(DustHipBodyQuery));
  FIELD(DustHipBodyQuery, struct_size); FIELD(DustHipBodyQuery, group); FIELD(DustHipBodyQuery, flags); FIELD(DustHipBodyQuery, palette);
  FIELD(DustHipBodyQuery, lo); FIELD(DustHipBodyQuery, hi); FIELD(DustHipBodyQuery, reserved);
  printf("DustHipBody %zu\n", sizeof(DustHipBody));
  FIELD(DustHipBody, key); FIELD(DustHipBody, voxels); FIELD(DustHipBody, lo); FIELD(DustHipBody, reserved0); FIELD(DustHipBody, hi);
  FIELD(DustHipBody, reserved1); FIELD(DustHipBody, mass); FIELD(DustHipBody, m1); FIELD(DustHipBody, m2);
  /* the query has a surface query's layout, with `group` where `faces` stands */
  printf("DustHipSurfaceQuery %zu\n", sizeof(DustHipSurfaceQuery));
  FIELD(DustHipSurfaceQuery, struct_size); FIELD(DustHipSurfaceQuery, faces); FIELD(DustHipSurfaceQuery, flags); FIELD(DustHipSurfaceQuery, palette);
  FIELD(DustHipSurfaceQuery, lo); FIELD(DustHipSurfaceQuery, hi); FIELD(DustHipSurfaceQuery, reserved);
  /* voxels, lo, hi and m1 stand where an island's voxels, lo, hi and sum would after the same header */
  FIELD(DustHipIsland, key); FIELD(DustHipIsland, voxels); FIELD(DustHipIsland, lo); FIELD(DustHipIsland, hi);
  CONSTANT(DUST_HIP_BODIES_ALL); CONSTANT(DUST_HIP_BODIES_MATERIALS); CONSTANT(DUST_HIP_BODIES_ISLANDS); CONSTANT(DUST_HIP_BODIES_CELLS);
  CONSTANT(DUST_HIP_BODY_WEIGHTS); CONSTANT(DUST_HIP_NO_CELL); CONSTANT(DUST_HIP_NO_ISLAND);
  return 0;
}
