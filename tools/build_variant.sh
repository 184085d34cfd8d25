#!/bin/bash
# build_variant.sh NAME [extra hipcc flags...]  -> build_ab/lib_NAME.so
# (FILE=pg_eval16.hip by default: that source recompiled with the extra flags, other objects
#  from the regular build)
set -e
cd "$(dirname "$0")/../posegen_amd/csrc"
name=$1; shift
src=${FILE:-pg_eval16.hip}
base=${src%.hip}
mkdir -p ../../build_ab
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -ffp-contract=on -fno-slp-vectorize"
/opt/rocm/bin/hipcc $FLAGS "$@" -c $src -o ../../build_ab/${base}_$name.o
objs=""
for f in ../_lib/obj/*.o; do          # every object of the regular build (the list of sources has one home, the Makefile)
  o=$(basename "$f" .o)
  if [ "$o" = "$base" ]; then objs="$objs ../../build_ab/${base}_$name.o"; else objs="$objs $f"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../build_ab/lib_$name.so $objs
echo built build_ab/lib_$name.so
