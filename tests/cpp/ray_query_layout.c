/* Prints sizeof / offsetof of the scene-query records of include/dust_hip.h, one "name value" per line (tests/test_ray_query_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  printf("DustHipRay %zu\n", sizeof(DustHipRay));
  FIELD(DustHipRay, origin); FIELD(DustHipRay, tmin); FIELD(DustHipRay, direction); FIELD(DustHipRay, tmax);
  printf("DustHipRayHit %zu\n", sizeof(DustHipRayHit));
  FIELD(DustHipRayHit, t); FIELD(DustHipRayHit, instance); FIELD(DustHipRayHit, block); FIELD(DustHipRayHit, voxel);
  FIELD(DustHipRayHit, xyz); FIELD(DustHipRayHit, face); FIELD(DustHipRayHit, palette); FIELD(DustHipRayHit, reserved);
  printf("DUST_HIP_NO_HIT %u\n", (unsigned)DUST_HIP_NO_HIT);
  printf("DUST_HIP_QUERY_ANY_HIT %u\n", (unsigned)DUST_HIP_QUERY_ANY_HIT);
  return 0;
}
