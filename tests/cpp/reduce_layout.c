/* Prints sizeof / offsetof of the reduce records of include/dust_hip.h and their constant, one "name value" per line
   (tests/test_reduce_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipReduce %zu\n", sizeof(DustHipReduce));
  FIELD(DustHipReduce, struct_size); FIELD(DustHipReduce, levels); FIELD(DustHipReduce, min_solid); FIELD(DustHipReduce, flags);
  printf("DustHipReduceResult %zu\n", sizeof(DustHipReduceResult));
  FIELD(DustHipReduceResult, src_voxels); FIELD(DustHipReduceResult, voxels); FIELD(DustHipReduceResult, extent);
  FIELD(DustHipReduceResult, reserved);
  CONSTANT(DUST_HIP_REDUCE_MAX_LEVELS);
  return 0;
}
