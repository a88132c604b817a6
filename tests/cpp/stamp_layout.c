/* Prints sizeof / offsetof of the stamp record of include/dust_hip.h and its constants, one "name value" per line
   (tests/test_stamp_witness.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  printf("DustHipStamp %zu\n", sizeof(DustHipStamp));
  FIELD(DustHipStamp, offset); FIELD(DustHipStamp, orient); FIELD(DustHipStamp, op); FIELD(DustHipStamp, src_lo); FIELD(DustHipStamp, pad0);
  FIELD(DustHipStamp, src_hi); FIELD(DustHipStamp, pad1); FIELD(DustHipStamp, reserved);
  printf("DUST_HIP_STAMP_PLACE %u\n", (unsigned)DUST_HIP_STAMP_PLACE);
  printf("DUST_HIP_STAMP_OVERWRITE %u\n", (unsigned)DUST_HIP_STAMP_OVERWRITE);
  printf("DUST_HIP_STAMP_REPLACE %u\n", (unsigned)DUST_HIP_STAMP_REPLACE);
  printf("DUST_HIP_STAMP_CARVE %u\n", (unsigned)DUST_HIP_STAMP_CARVE);
  printf("DUST_HIP_STAMP_PAINT %u\n", (unsigned)DUST_HIP_STAMP_PAINT);
  printf("DUST_HIP_MAX_STAMPS %u\n", (unsigned)DUST_HIP_MAX_STAMPS);
  return 0;
}
