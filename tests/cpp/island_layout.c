/* Prints sizeof / offsetof of the island records of include/dust_hip.h and their constants, one "name value" per line
   (tests/test_island_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  printf("DustHipIslandQuery %zu\n", sizeof(DustHipIslandQuery));
  FIELD(DustHipIslandQuery, struct_size); FIELD(DustHipIslandQuery, connectivity); FIELD(DustHipIslandQuery, anchor_lo);
  FIELD(DustHipIslandQuery, anchor_hi);
  printf("DustHipIsland %zu\n", sizeof(DustHipIsland));
  FIELD(DustHipIsland, key); FIELD(DustHipIsland, voxels); FIELD(DustHipIsland, lo); FIELD(DustHipIsland, flags);
  FIELD(DustHipIsland, hi); FIELD(DustHipIsland, reserved); FIELD(DustHipIsland, sum);
  printf("DUST_HIP_ISLANDS_FACES %u\n", (unsigned)DUST_HIP_ISLANDS_FACES);
  printf("DUST_HIP_ISLANDS_CORNERS %u\n", (unsigned)DUST_HIP_ISLANDS_CORNERS);
  printf("DUST_HIP_ISLAND_ANCHORED %u\n", (unsigned)DUST_HIP_ISLAND_ANCHORED);
  printf("DUST_HIP_NO_ISLAND %u\n", (unsigned)DUST_HIP_NO_ISLAND);
  printf("DUST_HIP_DETACH_KEEP_SOURCE %u\n", (unsigned)DUST_HIP_DETACH_KEEP_SOURCE);
  return 0;
}
