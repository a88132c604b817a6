/* Prints sizeof / offsetof of the census record of include/dust_hip.h and the call's constants, one "name value" per line
   (tests/test_census_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipCensus %zu\n", sizeof(DustHipCensus));
  FIELD(DustHipCensus, covered); FIELD(DustHipCensus, solid); FIELD(DustHipCensus, lo); FIELD(DustHipCensus, reserved0);
  FIELD(DustHipCensus, hi); FIELD(DustHipCensus, reserved1); FIELD(DustHipCensus, sum);
  printf("DustHipIsland %zu\n", sizeof(DustHipIsland));
  FIELD(DustHipIsland, lo); FIELD(DustHipIsland, hi); FIELD(DustHipIsland, sum);
  printf("DustHipEditShape %zu\n", sizeof(DustHipEditShape));
  CONSTANT(DUST_HIP_MAX_CENSUS_SHAPES);
  CONSTANT(DUST_HIP_MAX_CENSUS_TABLES);
  CONSTANT(DUST_HIP_CENSUS_BINS);
  return 0;
}
