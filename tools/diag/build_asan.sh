#!/bin/bash
# Sanitizer builds of the product's HOST code (kernels unchanged) and of the oracle, for crash hunting:
#   dust_amd/_asan/libdust_hip.so, dust_amd/_asan/liboracle.so   (run with tools/diag/with_asan.sh <command>)
set -e
cd "$(dirname "$0")/../.."
mkdir -p dust_amd/_asan
/opt/rocm/lib/llvm/bin/clang -fsanitize=address,undefined -shared-libsan -O1 -g -fPIC -shared -std=c11 -ffp-contract=off oracle/*.c -lm -o dust_amd/_asan/liboracle.so
# the product library through its own Makefile (one source list), host AddressSanitizer only: the kernels are compiled as they ship
san="-fsanitize=address -fno-gpu-sanitize -shared-libsan"
make -s -j8 -C dust_amd/csrc VARIANT=asan LIB=../_asan/libdust_hip.so EXTRA="-O1 -g $san" LDEXTRA="$san"
