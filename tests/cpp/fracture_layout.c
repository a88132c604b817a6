/* Prints sizeof / offsetof of the fracture records of include/dust_hip.h and the calls' constants, one "name value" per line
   (tests/test_fracture_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %lld\n", (long long)c)

int main(void) {
  printf("DustHipFractureSeed %zu\n", sizeof(DustHipFractureSeed));
  FIELD(DustHipFractureSeed, x); FIELD(DustHipFractureSeed, y); FIELD(DustHipFractureSeed, z); FIELD(DustHipFractureSeed, reserved);
  printf("DustHipFractureQuery %zu\n", sizeof(DustHipFractureQuery));
  FIELD(DustHipFractureQuery, struct_size); FIELD(DustHipFractureQuery, flags); FIELD(DustHipFractureQuery, palette); FIELD(DustHipFractureQuery, max_distance2);
  FIELD(DustHipFractureQuery, scale); FIELD(DustHipFractureQuery, reserved0); FIELD(DustHipFractureQuery, lo); FIELD(DustHipFractureQuery, hi);
  FIELD(DustHipFractureQuery, reserved);
  printf("DustHipFractureResult %zu\n", sizeof(DustHipFractureResult));
  FIELD(DustHipFractureResult, solid); FIELD(DustHipFractureResult, labelled); FIELD(DustHipFractureResult, cells); FIELD(DustHipFractureResult, largest_cell);
  FIELD(DustHipFractureResult, largest_voxels); FIELD(DustHipFractureResult, cut_faces); FIELD(DustHipFractureResult, max_d2); FIELD(DustHipFractureResult, lo);
  FIELD(DustHipFractureResult, reserved0); FIELD(DustHipFractureResult, hi); FIELD(DustHipFractureResult, reserved1); FIELD(DustHipFractureResult, reserved);
  printf("DustHipFractureCell %zu\n", sizeof(DustHipFractureCell));
  FIELD(DustHipFractureCell, voxels); FIELD(DustHipFractureCell, cut_faces); FIELD(DustHipFractureCell, lo); FIELD(DustHipFractureCell, reserved0);
  FIELD(DustHipFractureCell, hi); FIELD(DustHipFractureCell, reserved1); FIELD(DustHipFractureCell, sum);
  printf("DustHipCensus %zu\n", sizeof(DustHipCensus));
  FIELD(DustHipCensus, lo); FIELD(DustHipCensus, hi); FIELD(DustHipCensus, sum);
  CONSTANT(DUST_HIP_MAX_FRACTURE_SEEDS); CONSTANT(DUST_HIP_FRACTURE_SEED_MIN); CONSTANT(DUST_HIP_FRACTURE_SEED_MAX); CONSTANT(DUST_HIP_FRACTURE_MAX_SCALE);
  CONSTANT(DUST_HIP_FRACTURE_NO_LIMIT); CONSTANT(DUST_HIP_NO_CELL); CONSTANT(DUST_HIP_FRACTURE_SEAMS); CONSTANT(DUST_HIP_FRACTURE_LABELLED);
  CONSTANT(DUST_HIP_DETACH_KEEP_SOURCE);
  return 0;
}
