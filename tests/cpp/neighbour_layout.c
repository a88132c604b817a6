/* Prints sizeof / offsetof of the neighbours records of include/dust_hip.h and the calls' constants, one "name value" per line
   (tests/test_neighbour_abi.py). The surface query's offsets come along: a neighbours query has its layout. */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipNeighboursQuery %zu\n", sizeof(DustHipNeighboursQuery));
  FIELD(DustHipNeighboursQuery, struct_size); FIELD(DustHipNeighboursQuery, neighbourhood); FIELD(DustHipNeighboursQuery, flags);
  FIELD(DustHipNeighboursQuery, palette); FIELD(DustHipNeighboursQuery, lo); FIELD(DustHipNeighboursQuery, hi); FIELD(DustHipNeighboursQuery, birth);
  FIELD(DustHipNeighboursQuery, survive);
  printf("DustHipSurfaceQuery %zu\n", sizeof(DustHipSurfaceQuery));
  FIELD(DustHipSurfaceQuery, struct_size); FIELD(DustHipSurfaceQuery, faces); FIELD(DustHipSurfaceQuery, flags); FIELD(DustHipSurfaceQuery, palette);
  FIELD(DustHipSurfaceQuery, lo); FIELD(DustHipSurfaceQuery, hi); FIELD(DustHipSurfaceQuery, reserved);
  printf("DustHipNeighboursResult %zu\n", sizeof(DustHipNeighboursResult));
  FIELD(DustHipNeighboursResult, voxels); FIELD(DustHipNeighboursResult, solid); FIELD(DustHipNeighboursResult, born); FIELD(DustHipNeighboursResult, died);
  FIELD(DustHipNeighboursResult, lo); FIELD(DustHipNeighboursResult, pad0); FIELD(DustHipNeighboursResult, hi); FIELD(DustHipNeighboursResult, pad1);
  FIELD(DustHipNeighboursResult, reserved);
  printf("DustHipNeighboursApplied %zu\n", sizeof(DustHipNeighboursApplied));
  FIELD(DustHipNeighboursApplied, generations); FIELD(DustHipNeighboursApplied, solid_before); FIELD(DustHipNeighboursApplied, solid_after);
  FIELD(DustHipNeighboursApplied, reserved0); FIELD(DustHipNeighboursApplied, born); FIELD(DustHipNeighboursApplied, died); FIELD(DustHipNeighboursApplied, lo);
  FIELD(DustHipNeighboursApplied, pad0); FIELD(DustHipNeighboursApplied, hi); FIELD(DustHipNeighboursApplied, pad1); FIELD(DustHipNeighboursApplied, reserved);
  CONSTANT(DUST_HIP_NEIGHBOURS_FACES); CONSTANT(DUST_HIP_NEIGHBOURS_EDGES); CONSTANT(DUST_HIP_NEIGHBOURS_CORNERS); CONSTANT(DUST_HIP_NEIGHBOURS_WALLS);
  CONSTANT(DUST_HIP_NEIGHBOURS_MAJORITY); CONSTANT(DUST_HIP_NEIGHBOURS_BINS); CONSTANT(DUST_HIP_NEIGHBOURS_MAX_GENERATIONS); CONSTANT(DUST_HIP_SURFACE_WALLS);
  return 0;
}
