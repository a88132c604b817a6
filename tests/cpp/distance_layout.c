/* Prints sizeof / offsetof of the distance records of include/dust_hip.h and their constants, one "name value" per line
   (tests/test_distance_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipDistanceQuery %zu\n", sizeof(DustHipDistanceQuery));
  FIELD(DustHipDistanceQuery, struct_size); FIELD(DustHipDistanceQuery, target); FIELD(DustHipDistanceQuery, metric);
  FIELD(DustHipDistanceQuery, flags); FIELD(DustHipDistanceQuery, palette); FIELD(DustHipDistanceQuery, max_radius);
  FIELD(DustHipDistanceQuery, reserved);
  printf("DustHipDistanceResult %zu\n", sizeof(DustHipDistanceResult));
  FIELD(DustHipDistanceResult, targets); FIELD(DustHipDistanceResult, near); FIELD(DustHipDistanceResult, far);
  FIELD(DustHipDistanceResult, largest); FIELD(DustHipDistanceResult, largest_key); FIELD(DustHipDistanceResult, reserved);
  CONSTANT(DUST_HIP_DISTANCE_TO_SOLID); CONSTANT(DUST_HIP_DISTANCE_TO_EMPTY); CONSTANT(DUST_HIP_DISTANCE_TO_MATERIAL);
  CONSTANT(DUST_HIP_DISTANCE_EUCLIDEAN); CONSTANT(DUST_HIP_DISTANCE_CHEBYSHEV); CONSTANT(DUST_HIP_DISTANCE_WALLS);
  CONSTANT(DUST_HIP_DISTANCE_FAR); CONSTANT(DUST_HIP_DISTANCE_MAX_RADIUS); CONSTANT(DUST_HIP_DISTANCE_NO_KEY);
  return 0;
}
