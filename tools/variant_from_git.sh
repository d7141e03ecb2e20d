#!/bin/bash
# A/B reference: libdcp_var_<name>.so with one kernel unit (UNIT=stack_kernels.hip; default unwarp_kernels.hip) taken from a git revision
# (default HEAD) and everything else from the working tree (same C ABI, so the current Python binding loads it):
#   [UNIT=stack_kernels.hip] tools/variant_from_git.sh name [rev] ["-DFLAGS"]
# The revision must have the unit, and the same split of kernels over units as the working tree.  Build the library first.
case "${1:-}" in -h|--help) sed -n '2,5p' "$0" | sed 's/^# \{0,1\}//'; exit 0;; esac
set -e
N=$1; REV=${2:-HEAD}; FLAGS=${3:-}
UNIT=${UNIT:-unwarp_kernels.hip}
cd "$(dirname "$0")/../discorpy_amd/csrc"
git show $REV:discorpy_amd/csrc/$UNIT > /tmp/uk_$N.hip
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -I. $FLAGS -c /tmp/uk_$N.hip -o /tmp/uk_$N.o
OBJS=""
for o in $(make -s print-objs); do
  if [ "$o" = "../lib/${UNIT%.hip}.o" ]; then OBJS="$OBJS /tmp/uk_$N.o"; else OBJS="$OBJS $o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -Wl,--version-script=exports.map -o ../lib/libdcp_var_$N.so $OBJS -ldl
