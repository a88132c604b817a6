/* Prints sizeof / offsetof of the surface records of include/dust_hip.h and the calls' constants, one "name value" per line
   (tests/test_surface_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipSurfaceQuery %zu\n", sizeof(DustHipSurfaceQuery));
  FIELD(DustHipSurfaceQuery, struct_size); FIELD(DustHipSurfaceQuery, faces); FIELD(DustHipSurfaceQuery, flags); FIELD(DustHipSurfaceQuery, palette);
  FIELD(DustHipSurfaceQuery, lo); FIELD(DustHipSurfaceQuery, hi); FIELD(DustHipSurfaceQuery, reserved);
  printf("DustHipSurfaceResult %zu\n", sizeof(DustHipSurfaceResult));
  FIELD(DustHipSurfaceResult, voxels); FIELD(DustHipSurfaceResult, faces); FIELD(DustHipSurfaceResult, by_face); FIELD(DustHipSurfaceResult, solid);
  FIELD(DustHipSurfaceResult, lo); FIELD(DustHipSurfaceResult, pad0); FIELD(DustHipSurfaceResult, hi); FIELD(DustHipSurfaceResult, pad1);
  FIELD(DustHipSurfaceResult, reserved);
  printf("DustHipSurfaceVoxel %zu\n", sizeof(DustHipSurfaceVoxel));
  FIELD(DustHipSurfaceVoxel, key); FIELD(DustHipSurfaceVoxel, faces); FIELD(DustHipSurfaceVoxel, palette); FIELD(DustHipSurfaceVoxel, reserved);
  CONSTANT(DUST_HIP_FACE_NEG_X); CONSTANT(DUST_HIP_FACE_POS_X); CONSTANT(DUST_HIP_FACE_NEG_Y); CONSTANT(DUST_HIP_FACE_POS_Y);
  CONSTANT(DUST_HIP_FACE_NEG_Z); CONSTANT(DUST_HIP_FACE_POS_Z); CONSTANT(DUST_HIP_FACES_ALL);
  CONSTANT(DUST_HIP_SURFACE_WALLS); CONSTANT(DUST_HIP_SURFACE_BINS);
  return 0;
}
