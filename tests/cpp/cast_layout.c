/* Prints sizeof / offsetof of the cast records of include/dust_hip.h and their constants, one "name value" per line
   (tests/test_cast_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  printf("DustHipCast %zu\n", sizeof(DustHipCast));
  FIELD(DustHipCast, offset); FIELD(DustHipCast, orient); FIELD(DustHipCast, step); FIELD(DustHipCast, max_steps); FIELD(DustHipCast, flags);
  FIELD(DustHipCast, src_lo); FIELD(DustHipCast, pad0); FIELD(DustHipCast, src_hi); FIELD(DustHipCast, pad1); FIELD(DustHipCast, reserved);
  printf("DustHipCastHit %zu\n", sizeof(DustHipCastHit));
  FIELD(DustHipCastHit, steps); FIELD(DustHipCastHit, flags); FIELD(DustHipCastHit, contacts); FIELD(DustHipCastHit, voxels);
  FIELD(DustHipCastHit, contact); FIELD(DustHipCastHit, src_key);
  printf("DUST_HIP_CAST_WALLS %u\n", (unsigned)DUST_HIP_CAST_WALLS);
  printf("DUST_HIP_CAST_HIT %u\n", (unsigned)DUST_HIP_CAST_HIT);
  printf("DUST_HIP_CAST_OVERLAP %u\n", (unsigned)DUST_HIP_CAST_OVERLAP);
  printf("DUST_HIP_CAST_HIT_WALL %u\n", (unsigned)DUST_HIP_CAST_HIT_WALL);
  printf("DUST_HIP_CAST_MAX_STEPS %u\n", (unsigned)DUST_HIP_CAST_MAX_STEPS);
  printf("DUST_HIP_MAX_CASTS %u\n", (unsigned)DUST_HIP_MAX_CASTS);
  printf("DUST_HIP_CAST_NO_KEY %u\n", (unsigned)DUST_HIP_CAST_NO_KEY);
  return 0;
}
