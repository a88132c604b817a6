/* Prints sizeof / offsetof of the records of dust_hip_model_read_hierarchy (include/dust_hip.h) and its constants, one "name value" per
   line (tests/test_hierarchy_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipHierarchyInfo %zu\n", sizeof(DustHipHierarchyInfo));
  FIELD(DustHipHierarchyInfo, struct_size); FIELD(DustHipHierarchyInfo, extent_log2); FIELD(DustHipHierarchyInfo, n_mid);
  FIELD(DustHipHierarchyInfo, n_l2); FIELD(DustHipHierarchyInfo, bmin); FIELD(DustHipHierarchyInfo, bmax); FIELD(DustHipHierarchyInfo, reserved);
  printf("DustHipMidNode %zu\n", sizeof(DustHipMidNode));
  FIELD(DustHipMidNode, mask_lo); FIELD(DustHipMidNode, mask_hi); FIELD(DustHipMidNode, first_block); FIELD(DustHipMidNode, pad);
  printf("DustHipL2Cell %zu\n", sizeof(DustHipL2Cell));
  FIELD(DustHipL2Cell, mid); FIELD(DustHipL2Cell, bounds); FIELD(DustHipL2Cell, child_mask);
  CONSTANT(DUST_HIP_N16_BYTES); CONSTANT(DUST_HIP_N16_ROOT_BYTES);
  return 0;
}
