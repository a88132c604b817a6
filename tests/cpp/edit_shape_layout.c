/* Prints sizeof / offsetof of the shape-edit record of include/dust_hip.h and its constants, one "name value" per line
   (tests/test_shape_edit_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  printf("DustHipEditShape %zu\n", sizeof(DustHipEditShape));
  FIELD(DustHipEditShape, a); FIELD(DustHipEditShape, kind); FIELD(DustHipEditShape, b); FIELD(DustHipEditShape, radius);
  FIELD(DustHipEditShape, op); FIELD(DustHipEditShape, palette); FIELD(DustHipEditShape, reserved);
  printf("DUST_HIP_SHAPE_BOX %u\n", (unsigned)DUST_HIP_SHAPE_BOX);
  printf("DUST_HIP_SHAPE_SPHERE %u\n", (unsigned)DUST_HIP_SHAPE_SPHERE);
  printf("DUST_HIP_SHAPE_CAPSULE %u\n", (unsigned)DUST_HIP_SHAPE_CAPSULE);
  printf("DUST_HIP_EDIT_CARVE %u\n", (unsigned)DUST_HIP_EDIT_CARVE);
  printf("DUST_HIP_EDIT_FILL %u\n", (unsigned)DUST_HIP_EDIT_FILL);
  printf("DUST_HIP_EDIT_PAINT %u\n", (unsigned)DUST_HIP_EDIT_PAINT);
  printf("DUST_HIP_EDIT_PLACE %u\n", (unsigned)DUST_HIP_EDIT_PLACE);
  printf("DUST_HIP_MAX_EDIT_SHAPES %u\n", (unsigned)DUST_HIP_MAX_EDIT_SHAPES);
  return 0;
}
