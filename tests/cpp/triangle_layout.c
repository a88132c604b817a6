/* Prints sizeof / offsetof of the voxelisation records of include/dust_hip.h and the calls' constants, one "name value" per line
   (tests/test_triangle_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipTriangle %zu\n", sizeof(DustHipTriangle));
  FIELD(DustHipTriangle, v); FIELD(DustHipTriangle, op); FIELD(DustHipTriangle, palette); FIELD(DustHipTriangle, reserved);
  printf("DustHipFillMeshQuery %zu\n", sizeof(DustHipFillMeshQuery));
  FIELD(DustHipFillMeshQuery, struct_size); FIELD(DustHipFillMeshQuery, op); FIELD(DustHipFillMeshQuery, palette); FIELD(DustHipFillMeshQuery, flags);
  FIELD(DustHipFillMeshQuery, lo); FIELD(DustHipFillMeshQuery, hi); FIELD(DustHipFillMeshQuery, reserved);
  printf("DustHipFillMeshResult %zu\n", sizeof(DustHipFillMeshResult));
  FIELD(DustHipFillMeshResult, covered); FIELD(DustHipFillMeshResult, changed); FIELD(DustHipFillMeshResult, live); FIELD(DustHipFillMeshResult, crossing);
  FIELD(DustHipFillMeshResult, lo); FIELD(DustHipFillMeshResult, hi); FIELD(DustHipFillMeshResult, reserved);
  CONSTANT(DUST_HIP_TRIANGLE_UNIT); CONSTANT(DUST_HIP_TRIANGLE_MAX_COORD); CONSTANT(DUST_HIP_MAX_EDIT_TRIANGLES); CONSTANT(DUST_HIP_MAX_MESH_TRIANGLES);
  CONSTANT(DUST_HIP_EDIT_CARVE); CONSTANT(DUST_HIP_EDIT_FILL); CONSTANT(DUST_HIP_EDIT_PAINT); CONSTANT(DUST_HIP_EDIT_PLACE);
  return 0;
}
