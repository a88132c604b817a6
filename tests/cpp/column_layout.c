/* Prints sizeof / offsetof of the columns records of include/dust_hip.h and the calls' constants, one "name value" per line
   (tests/test_column_abi.py). The surface query's offsets come along: a columns query has its layout. */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipColumnsQuery %zu\n", sizeof(DustHipColumnsQuery));
  FIELD(DustHipColumnsQuery, struct_size); FIELD(DustHipColumnsQuery, face); FIELD(DustHipColumnsQuery, flags); FIELD(DustHipColumnsQuery, palette);
  FIELD(DustHipColumnsQuery, lo); FIELD(DustHipColumnsQuery, hi); FIELD(DustHipColumnsQuery, layer); FIELD(DustHipColumnsQuery, reserved);
  printf("DustHipSurfaceQuery %zu\n", sizeof(DustHipSurfaceQuery));
  FIELD(DustHipSurfaceQuery, struct_size); FIELD(DustHipSurfaceQuery, faces); FIELD(DustHipSurfaceQuery, flags); FIELD(DustHipSurfaceQuery, palette);
  FIELD(DustHipSurfaceQuery, lo); FIELD(DustHipSurfaceQuery, hi); FIELD(DustHipSurfaceQuery, reserved);
  printf("DustHipColumnsResult %zu\n", sizeof(DustHipColumnsResult));
  FIELD(DustHipColumnsResult, columns); FIELD(DustHipColumnsResult, hit); FIELD(DustHipColumnsResult, voxels); FIELD(DustHipColumnsResult, runs);
  FIELD(DustHipColumnsResult, depth_sum); FIELD(DustHipColumnsResult, nearest_key); FIELD(DustHipColumnsResult, farthest_key);
  FIELD(DustHipColumnsResult, lo); FIELD(DustHipColumnsResult, pad0); FIELD(DustHipColumnsResult, hi); FIELD(DustHipColumnsResult, pad1);
  FIELD(DustHipColumnsResult, reserved);
  printf("DustHipColumnCell %zu\n", sizeof(DustHipColumnCell));
  FIELD(DustHipColumnCell, at); FIELD(DustHipColumnCell, palette); FIELD(DustHipColumnCell, length_minus_1); FIELD(DustHipColumnCell, runs);
  CONSTANT(DUST_HIP_COLUMNS_RUN); CONSTANT(DUST_HIP_COLUMNS_GAP); CONSTANT(DUST_HIP_COLUMNS_BINS); CONSTANT(DUST_HIP_COLUMNS_NO_KEY);
  CONSTANT(DUST_HIP_FACE_NEG_X); CONSTANT(DUST_HIP_FACE_POS_X); CONSTANT(DUST_HIP_FACE_NEG_Y); CONSTANT(DUST_HIP_FACE_POS_Y);
  CONSTANT(DUST_HIP_FACE_NEG_Z); CONSTANT(DUST_HIP_FACE_POS_Z);
  return 0;
}
