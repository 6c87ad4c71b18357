#!/bin/bash
# build an alternate engine library for same-box A/B timing: tools/build_variant.sh <name> [extra hipcc flags...]
# -> build/ab/libfreud_sae_<name>.so   (compare with tools/ab_bench.sh)
# Through the Makefile (every translation unit, its flags, one link), with the variant's own object directory; the extra flags
# come last, so a diagnostic build that warns can pass -Wno-error.
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$root/build/ab"
make -C "$root/freud_amd/csrc" -j "${MAX_JOBS:-16}" OUT="$root/build/ab/libfreud_sae_$name.so" OBJDIR="$root/build/ab/obj_$name" \
  EXTRA_CXXFLAGS="$*" "$root/build/ab/libfreud_sae_$name.so"
echo build/ab/libfreud_sae_$name.so
