#!/bin/bash
# Builds experiment variants of the library into discorpy_amd/lib/variants/lib_<name>.so (what tools/ab_variants.sh alternates):
#   tools/variants.sh name "-DFLAG=.." [name2 "-D.."] ...
# FILE=stack_kernels.hip tools/variants.sh ...  rebuilds that translation unit (any *.hip of the library) instead of unwarp_kernels.hip.
# The other objects are the library's own, as the Makefile lists them (`make print-objs`): build the library first.
case "${1:-}" in -h|--help) sed -n '2,5p' "$0" | sed 's/^# \{0,1\}//'; exit 0;; esac
set -e
cd "$(dirname "$0")/../discorpy_amd/csrc"
FILE=${FILE:-unwarp_kernels.hip}
BASE=${FILE%.hip}
ALL=$(make -s print-objs)
case " $(echo $ALL) " in *" ../lib/$BASE.o "*) ;; *) echo "variants.sh: $FILE is not a unit of the library" >&2; exit 1;; esac
while [ $# -ge 2 ]; do
  n=$1; f=$2; shift 2
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden $f -c $FILE -o /tmp/var_$n.o
  OBJS=""
  for o in $ALL; do
    if [ "$o" = "../lib/$BASE.o" ]; then OBJS="$OBJS /tmp/var_$n.o"; else OBJS="$OBJS $o"; fi
  done
  mkdir -p ../lib/variants
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -Wl,--version-script=exports.map -o ../lib/variants/lib_$n.so $OBJS -ldl
done
