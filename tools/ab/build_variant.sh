#!/bin/bash
# Build a variant of the library for same-box A/B timing (no GPU needed):
#   tools/ab/build_variant.sh NAME "-DSOME_SWITCH" [UNIT.hip]  ->  tools/ab/libvus_n_NAME.so (plain) and, when UNIT is
#   band_solve.hip (the default; the only unit with -DVUS_TIMING marks), libvus_t_NAME.so (-DVUS_TIMING)
# Only UNIT is rebuilt, with the plain flags (the front-end units / ransac.hip have theirs: build_frontend_variant.sh); the other
# objects are those `make` built in visual-underwater-slam_amd/csrc (run it there first), named by `make print-objs`.
# The .so files are git-ignored; delete them when the experiment is over.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
cd "$HERE/../../visual-underwater-slam_amd/csrc"
name=$1; flags=$2; unit=${3:-band_solve.hip}
obj=${unit%.hip}.o
OFFLOAD=$(make -s print-offload)          # the one place that names the target and the objects: csrc/Makefile
OBJS=" $(make -s print-objs) "
case "$OBJS" in *" $obj "*) ;; *) echo "build_variant.sh: $unit is not a unit of the library ($OBJS)" >&2; exit 1 ;; esac
mkdir -p /tmp/tb_$name
rm -f "$HERE/libvus_n_$name.so" "$HERE/libvus_t_$name.so"     # a failed build must not leave an older binary to be timed
kinds=n; [ $unit = band_solve.hip ] && kinds="n t"
pids=()
for kind in $kinds; do
  extra=""; [ $kind = t ] && extra="-DVUS_TIMING"
  ( /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC $OFFLOAD -Wno-unused-function $extra $flags -c $unit -o /tmp/tb_$name/$kind.o \
    && /opt/rocm/bin/hipcc -shared -fPIC $OFFLOAD ${OBJS/ $obj / /tmp/tb_$name/$kind.o } -o "$HERE/libvus_${kind}_$name.so" ) &
  pids+=($!)
done
for pid in "${pids[@]}"; do
  wait "$pid" || { echo "build_variant.sh: building variant '$name' failed" >&2; exit 1; }
done
