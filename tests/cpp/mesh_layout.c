/* Prints sizeof / offsetof of the mesh records of include/dust_hip.h and the call's constants, one "name value" per line
   (tests/test_mesh_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipMeshQuery %zu\n", sizeof(DustHipMeshQuery));
  FIELD(DustHipMeshQuery, struct_size); FIELD(DustHipMeshQuery, faces); FIELD(DustHipMeshQuery, flags); FIELD(DustHipMeshQuery, palette);
  FIELD(DustHipMeshQuery, lo); FIELD(DustHipMeshQuery, hi); FIELD(DustHipMeshQuery, reserved);
  printf("DustHipMeshQuad %zu\n", sizeof(DustHipMeshQuad));
  FIELD(DustHipMeshQuad, key); FIELD(DustHipMeshQuad, face); FIELD(DustHipMeshQuad, palette); FIELD(DustHipMeshQuad, du); FIELD(DustHipMeshQuad, dv);
  printf("DustHipMeshResult %zu\n", sizeof(DustHipMeshResult));
  FIELD(DustHipMeshResult, quads); FIELD(DustHipMeshResult, faces); FIELD(DustHipMeshResult, quads_by_face); FIELD(DustHipMeshResult, faces_by_face);
  FIELD(DustHipMeshResult, largest); FIELD(DustHipMeshResult, reserved);
  /* the query is a surface query field for field */
  printf("DustHipSurfaceQuery %zu\n", sizeof(DustHipSurfaceQuery));
  FIELD(DustHipSurfaceQuery, struct_size); FIELD(DustHipSurfaceQuery, faces); FIELD(DustHipSurfaceQuery, flags); FIELD(DustHipSurfaceQuery, palette);
  FIELD(DustHipSurfaceQuery, lo); FIELD(DustHipSurfaceQuery, hi); FIELD(DustHipSurfaceQuery, reserved);
  CONSTANT(DUST_HIP_MESH_WALLS); CONSTANT(DUST_HIP_MESH_ANY_PALETTE); CONSTANT(DUST_HIP_SURFACE_WALLS); CONSTANT(DUST_HIP_FACES_ALL);
  return 0;
}
