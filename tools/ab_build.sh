#!/bin/bash
# Build the current tree into noisereduce_amd/_ab/lib_<tag>.so (cross-compiling here) with the flags of
# __graft_entry__.build(); run variants on the GPU box with
#   for f in noisereduce_amd/_ab/*.so; do SG_LIB_PATH=$PWD/$f python tools/time_onepass.py; done
# usage: tools/ab_build.sh <tag> [extra hipcc flags]
# The extra flags go to the units named in AB_UNITS (default: api.hip, the gate engine: the one unit that includes the gate's
# kernel headers; create.hip, debug.hip and shims.hip are host code only, the table-driven paths have units of their own);
# the other units' objects are built once without them into noisereduce_amd/_ab/obj/ and reused while newer than
# everything they include.
set -e
cd "$(dirname "$0")/.."
TAG=$1; shift
AB_UNITS=${AB_UNITS:-api.hip}
mkdir -p noisereduce_amd/_ab/obj
OBJ=$PWD/noisereduce_amd/_ab/obj
cd noisereduce_amd/csrc
CC="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Xclang -target-feature -Xclang -packed-fp32-ops"
stale() {  # object missing, or older than a file of its dependency list (written by -MD when it was built)
  [ -e $1 ] && [ -e ${1%.o}.d ] || return 0
  for d in $(sed -e 's/^[^:]*://' -e 's/\\$//' ${1%.o}.d); do [ $d -nt $1 ] && return 0; done
  return 1
}
objs=""
for u in *.hip; do
  case " $AB_UNITS " in
    *" $u "*) o=$OBJ/${u%.hip}_$TAG.o; $CC -c $u -o $o "$@" 2>$OBJ/${u%.hip}_$TAG.log & ;;
    *) o=$OBJ/${u%.hip}.o; if stale $o; then $CC -c $u -o $o -MD -MF ${o%.o}.d 2>/dev/null & fi ;;
  esac
  objs="$objs $o"
done
wait
$CC -shared -Wl,--version-script=exports.map $objs -o ../_ab/lib_$TAG.so -ldl
ls -la ../_ab/lib_$TAG.so
