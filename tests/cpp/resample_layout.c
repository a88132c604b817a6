/* Prints sizeof / offsetof of the resample records of include/dust_hip.h and the call's constants, one "name value" per line
   (tests/test_resample_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %lld\n", (long long)c)

int main(void) {
  printf("DustHipResample %zu\n", sizeof(DustHipResample));
  FIELD(DustHipResample, m); FIELD(DustHipResample, t); FIELD(DustHipResample, dst_lo); FIELD(DustHipResample, dst_hi); FIELD(DustHipResample, src_lo);
  FIELD(DustHipResample, pad0); FIELD(DustHipResample, src_hi); FIELD(DustHipResample, pad1); FIELD(DustHipResample, op); FIELD(DustHipResample, reserved);
  printf("DustHipResampleCount %zu\n", sizeof(DustHipResampleCount));
  FIELD(DustHipResampleCount, changed); FIELD(DustHipResampleCount, covered); FIELD(DustHipResampleCount, solid); FIELD(DustHipResampleCount, blocked);
  printf("DustHipStamp %zu\n", sizeof(DustHipStamp));
  CONSTANT(DUST_HIP_RESAMPLE_ONE); CONSTANT(DUST_HIP_RESAMPLE_MAX_M); CONSTANT(DUST_HIP_RESAMPLE_MAX_T); CONSTANT(DUST_HIP_RESAMPLE_DRY_RUN);
  CONSTANT(DUST_HIP_MAX_RESAMPLES); CONSTANT(DUST_HIP_STAMP_PLACE); CONSTANT(DUST_HIP_STAMP_OVERWRITE); CONSTANT(DUST_HIP_STAMP_REPLACE);
  CONSTANT(DUST_HIP_STAMP_CARVE); CONSTANT(DUST_HIP_STAMP_PAINT);
  return 0;
}
