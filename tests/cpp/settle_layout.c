/* Prints sizeof / offsetof of the settle records of include/dust_hip.h and the calls' constants, one "name value" per line
   (tests/test_settle_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipSettleQuery %zu\n", sizeof(DustHipSettleQuery));
  FIELD(DustHipSettleQuery, struct_size); FIELD(DustHipSettleQuery, toward); FIELD(DustHipSettleQuery, flags); FIELD(DustHipSettleQuery, reserved);
  FIELD(DustHipSettleQuery, lo); FIELD(DustHipSettleQuery, hi); FIELD(DustHipSettleQuery, loose);
  printf("DustHipSettleResult %zu\n", sizeof(DustHipSettleResult));
  FIELD(DustHipSettleResult, columns); FIELD(DustHipSettleResult, loose); FIELD(DustHipSettleResult, fixed); FIELD(DustHipSettleResult, moved);
  FIELD(DustHipSettleResult, changed); FIELD(DustHipSettleResult, fall_max); FIELD(DustHipSettleResult, fall_sum); FIELD(DustHipSettleResult, lo);
  FIELD(DustHipSettleResult, pad0); FIELD(DustHipSettleResult, hi); FIELD(DustHipSettleResult, pad1); FIELD(DustHipSettleResult, changed_columns);
  FIELD(DustHipSettleResult, reserved);
  printf("DustHipSettleApplied %zu\n", sizeof(DustHipSettleApplied));
  FIELD(DustHipSettleApplied, generations); FIELD(DustHipSettleApplied, first_moved); FIELD(DustHipSettleApplied, loose); FIELD(DustHipSettleApplied, reserved0);
  FIELD(DustHipSettleApplied, slid); FIELD(DustHipSettleApplied, fell); FIELD(DustHipSettleApplied, fall_sum); FIELD(DustHipSettleApplied, lo);
  FIELD(DustHipSettleApplied, pad0); FIELD(DustHipSettleApplied, hi); FIELD(DustHipSettleApplied, pad1); FIELD(DustHipSettleApplied, reserved);
  CONSTANT(DUST_HIP_SETTLE_MAX_GENERATIONS); CONSTANT(DUST_HIP_FACE_NEG_X); CONSTANT(DUST_HIP_FACE_POS_X); CONSTANT(DUST_HIP_FACE_NEG_Y);
  CONSTANT(DUST_HIP_FACE_POS_Y); CONSTANT(DUST_HIP_FACE_NEG_Z); CONSTANT(DUST_HIP_FACE_POS_Z);
  return 0;
}
