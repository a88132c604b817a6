/* Prints sizeof / offsetof of the delta records of include/dust_hip.h and the calls' constants, one "name value" per line
   (tests/test_delta_abi.py). The surface query's offsets come along: a delta query has its layout. */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipDeltaQuery %zu\n", sizeof(DustHipDeltaQuery));
  FIELD(DustHipDeltaQuery, struct_size); FIELD(DustHipDeltaQuery, kinds); FIELD(DustHipDeltaQuery, flags); FIELD(DustHipDeltaQuery, palette);
  FIELD(DustHipDeltaQuery, lo); FIELD(DustHipDeltaQuery, hi); FIELD(DustHipDeltaQuery, reserved);
  printf("DustHipSurfaceQuery %zu\n", sizeof(DustHipSurfaceQuery));
  FIELD(DustHipSurfaceQuery, struct_size); FIELD(DustHipSurfaceQuery, faces); FIELD(DustHipSurfaceQuery, flags); FIELD(DustHipSurfaceQuery, palette);
  FIELD(DustHipSurfaceQuery, lo); FIELD(DustHipSurfaceQuery, hi); FIELD(DustHipSurfaceQuery, reserved);
  printf("DustHipDeltaResult %zu\n", sizeof(DustHipDeltaResult));
  FIELD(DustHipDeltaResult, voxels); FIELD(DustHipDeltaResult, added); FIELD(DustHipDeltaResult, removed); FIELD(DustHipDeltaResult, repainted);
  FIELD(DustHipDeltaResult, solid_before); FIELD(DustHipDeltaResult, solid_after);
  FIELD(DustHipDeltaResult, lo); FIELD(DustHipDeltaResult, pad0); FIELD(DustHipDeltaResult, hi); FIELD(DustHipDeltaResult, pad1);
  FIELD(DustHipDeltaResult, reserved);
  printf("DustHipDeltaVoxel %zu\n", sizeof(DustHipDeltaVoxel));
  FIELD(DustHipDeltaVoxel, key); FIELD(DustHipDeltaVoxel, kind); FIELD(DustHipDeltaVoxel, before); FIELD(DustHipDeltaVoxel, after);
  FIELD(DustHipDeltaVoxel, reserved);
  CONSTANT(DUST_HIP_DELTA_ADDED); CONSTANT(DUST_HIP_DELTA_REMOVED); CONSTANT(DUST_HIP_DELTA_REPAINTED); CONSTANT(DUST_HIP_DELTA_ALL);
  CONSTANT(DUST_HIP_DELTA_NONE); CONSTANT(DUST_HIP_DELTA_BACKWARD); CONSTANT(DUST_HIP_DELTA_BINS); CONSTANT(DUST_HIP_MAX_DELTA_RECORDS);
  return 0;
}
