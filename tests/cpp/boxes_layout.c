/* Prints sizeof / offsetof of the boxes records of include/dust_hip.h and the call's constants, one "name value" per line
   (tests/test_boxes_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipBoxesQuery %zu\n", sizeof(DustHipBoxesQuery));
  FIELD(DustHipBoxesQuery, struct_size); FIELD(DustHipBoxesQuery, axis); FIELD(DustHipBoxesQuery, flags); FIELD(DustHipBoxesQuery, palette);
  FIELD(DustHipBoxesQuery, lo); FIELD(DustHipBoxesQuery, hi); FIELD(DustHipBoxesQuery, reserved);
  printf("DustHipBox %zu\n", sizeof(DustHipBox));
  FIELD(DustHipBox, key); FIELD(DustHipBox, palette); FIELD(DustHipBox, dx); FIELD(DustHipBox, dy); FIELD(DustHipBox, dz);
  printf("DustHipBoxesResult %zu\n", sizeof(DustHipBoxesResult));
  FIELD(DustHipBoxesResult, boxes); FIELD(DustHipBoxesResult, rects); FIELD(DustHipBoxesResult, voxels); FIELD(DustHipBoxesResult, lo);
  FIELD(DustHipBoxesResult, pad0); FIELD(DustHipBoxesResult, hi); FIELD(DustHipBoxesResult, pad1); FIELD(DustHipBoxesResult, reserved);
  /* the query has a surface query's layout, with `axis` where `faces` stands */
  printf("DustHipSurfaceQuery %zu\n", sizeof(DustHipSurfaceQuery));
  FIELD(DustHipSurfaceQuery, struct_size); FIELD(DustHipSurfaceQuery, faces); FIELD(DustHipSurfaceQuery, flags); FIELD(DustHipSurfaceQuery, palette);
  FIELD(DustHipSurfaceQuery, lo); FIELD(DustHipSurfaceQuery, hi); FIELD(DustHipSurfaceQuery, reserved);
  CONSTANT(DUST_HIP_BOXES_ANY_PALETTE); CONSTANT(DUST_HIP_MAX_EDIT_SHAPES);
  return 0;
}
