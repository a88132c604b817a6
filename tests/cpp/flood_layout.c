/* Prints sizeof / offsetof of the flood records of include/dust_hip.h and their constants, one "name value" per line
   (tests/test_flood_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  printf("DustHipFloodQuery %zu\n", sizeof(DustHipFloodQuery));
  FIELD(DustHipFloodQuery, struct_size); FIELD(DustHipFloodQuery, medium); FIELD(DustHipFloodQuery, palette);
  FIELD(DustHipFloodQuery, max_steps); FIELD(DustHipFloodQuery, lo); FIELD(DustHipFloodQuery, hi);
  printf("DustHipFloodResult %zu\n", sizeof(DustHipFloodResult));
  FIELD(DustHipFloodResult, reached); FIELD(DustHipFloodResult, farthest); FIELD(DustHipFloodResult, seeds_used);
  FIELD(DustHipFloodResult, boundary); FIELD(DustHipFloodResult, lo); FIELD(DustHipFloodResult, pad0); FIELD(DustHipFloodResult, hi);
  FIELD(DustHipFloodResult, pad1); FIELD(DustHipFloodResult, reserved);
  printf("DUST_HIP_FLOOD_EMPTY %u\n", (unsigned)DUST_HIP_FLOOD_EMPTY);
  printf("DUST_HIP_FLOOD_SOLID %u\n", (unsigned)DUST_HIP_FLOOD_SOLID);
  printf("DUST_HIP_FLOOD_MATERIAL %u\n", (unsigned)DUST_HIP_FLOOD_MATERIAL);
  printf("DUST_HIP_FLOOD_UNREACHED %u\n", (unsigned)DUST_HIP_FLOOD_UNREACHED);
  printf("DUST_HIP_FLOOD_MAX_STEPS %u\n", (unsigned)DUST_HIP_FLOOD_MAX_STEPS);
  printf("DUST_HIP_MAX_FLOOD_SEEDS %u\n", (unsigned)DUST_HIP_MAX_FLOOD_SEEDS);
  return 0;
}
