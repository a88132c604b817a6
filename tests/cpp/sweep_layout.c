/* Prints sizeof / offsetof of the scene box-sweep records of include/dust_hip.h, one "name value" per line (tests/test_sweep_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  printf("DustHipBoxSweep %zu\n", sizeof(DustHipBoxSweep));
  FIELD(DustHipBoxSweep, lo); FIELD(DustHipBoxSweep, reserved0); FIELD(DustHipBoxSweep, hi); FIELD(DustHipBoxSweep, reserved1);
  FIELD(DustHipBoxSweep, delta); FIELD(DustHipBoxSweep, reserved2);
  printf("DustHipSweepHit %zu\n", sizeof(DustHipSweepHit));
  FIELD(DustHipSweepHit, t); FIELD(DustHipSweepHit, instance); FIELD(DustHipSweepHit, block); FIELD(DustHipSweepHit, xyz);
  FIELD(DustHipSweepHit, palette); FIELD(DustHipSweepHit, voxel); FIELD(DustHipSweepHit, normal);
  printf("DUST_HIP_QUERY_ANY_HIT %u\n", (unsigned)DUST_HIP_QUERY_ANY_HIT);
  printf("DUST_HIP_SWEEP_IGNORE_START %u\n", (unsigned)DUST_HIP_SWEEP_IGNORE_START);
  printf("DUST_HIP_NO_HIT %u\n", (unsigned)DUST_HIP_NO_HIT);
  return 0;
}
