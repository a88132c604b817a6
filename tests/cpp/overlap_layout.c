/* Prints sizeof / offsetof of the scene box-query records of include/dust_hip.h, one "name value" per line (tests/test_overlap_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  printf("DustHipBoxQuery %zu\n", sizeof(DustHipBoxQuery));
  FIELD(DustHipBoxQuery, lo); FIELD(DustHipBoxQuery, first); FIELD(DustHipBoxQuery, hi); FIELD(DustHipBoxQuery, capacity);
  printf("DustHipVoxelRef %zu\n", sizeof(DustHipVoxelRef));
  FIELD(DustHipVoxelRef, instance); FIELD(DustHipVoxelRef, block); FIELD(DustHipVoxelRef, xyz); FIELD(DustHipVoxelRef, palette);
  FIELD(DustHipVoxelRef, voxel);
  printf("DUST_HIP_QUERY_ANY_HIT %u\n", (unsigned)DUST_HIP_QUERY_ANY_HIT);
  return 0;
}
