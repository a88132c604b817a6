/* Prints sizeof / offsetof of the joint records of include/dust_hip.h and the call's constants, one "name value" per line
   (tests/test_joints_abi.py). */
#include <stddef.h>
#include <stdio.h>

#include "dust_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define CONSTANT(c) printf(#c " %u\n", (unsigned)c)

int main(void) {
  printf("DustHipJointQuery %zu\n", sizeof(DustHipJointQuery));
  FIELD(DustHipJointQuery, struct_size); FIELD(DustHipJointQuery, group); FIELD(DustHipJointQuery, flags); FIELD(DustHipJointQuery, palette);
  FIELD(DustHipJointQuery, lo); FIELD(DustHipJointQuery, hi); FIELD(DustHipJointQuery, reserved);
  printf("DustHipJoint %zu\n", sizeof(DustHipJoint));
  FIELD(DustHipJoint, a); FIELD(DustHipJoint, b); FIELD(DustHipJoint, faces); FIELD(DustHipJoint, reserved0); FIELD(DustHipJoint, by_face);
  FIELD(DustHipJoint, lo2); FIELD(DustHipJoint, hi2); FIELD(DustHipJoint, reserved1); FIELD(DustHipJoint, sum2);
  /* the query has a surface query's layout, with `group` where `faces` stands */
  printf("DustHipSurfaceQuery %zu\n", sizeof(DustHipSurfaceQuery));
  FIELD(DustHipSurfaceQuery, struct_size); FIELD(DustHipSurfaceQuery, faces); FIELD(DustHipSurfaceQuery, flags); FIELD(DustHipSurfaceQuery, palette);
  FIELD(DustHipSurfaceQuery, lo); FIELD(DustHipSurfaceQuery, hi); FIELD(DustHipSurfaceQuery, reserved);
  CONSTANT(DUST_HIP_JOINTS_MATERIALS); CONSTANT(DUST_HIP_JOINTS_CELLS); CONSTANT(DUST_HIP_JOINT_REST); CONSTANT(DUST_HIP_NO_CELL);
  CONSTANT(DUST_HIP_FACE_NEG_X); CONSTANT(DUST_HIP_FACE_POS_X); CONSTANT(DUST_HIP_FACE_NEG_Y); CONSTANT(DUST_HIP_FACE_POS_Y);
  CONSTANT(DUST_HIP_FACE_NEG_Z); CONSTANT(DUST_HIP_FACE_POS_Z);
  return 0;
}
