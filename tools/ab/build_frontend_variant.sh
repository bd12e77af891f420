#!/bin/bash
# Front-end twin of build_variant.sh: tools/ab/build_frontend_variant.sh NAME "-DSWITCH ..." [UNIT.hip] -> tools/ab/libvus_fe_NAME.so
# (UNIT, detect.hip unless named, rebuilt with the switches and the front-end flags; the other objects from
# visual-underwater-slam_amd/csrc; select it with VUS_HIP_LIB).
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
cd "$HERE/../../visual-underwater-slam_amd/csrc"
name=$1; flags=$2; unit=${3:-detect.hip}
stem=${unit%.hip}
OFFLOAD=$(make -s print-offload)
OBJS=" $(make -s print-objs) "
case "$OBJS" in *" $stem.o "*) ;; *) echo "build_frontend_variant.sh: $unit is not a unit of the library ($OBJS)" >&2; exit 1 ;; esac
mkdir -p /tmp/tb_fe_$name
rm -f "$HERE/libvus_fe_$name.so"
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC $OFFLOAD -Wno-unused-function $(make -s print-frontend-flags) $flags -c $unit -o /tmp/tb_fe_$name/$stem.o
/opt/rocm/bin/hipcc -shared -fPIC $OFFLOAD ${OBJS/ $stem.o / /tmp/tb_fe_$name/$stem.o } -o "$HERE/libvus_fe_$name.so"
[ $stem = detect ] || exit 0
/opt/rocm/bin/hipcc -O3 -std=c++17 $OFFLOAD $(make -s print-frontend-flags) $flags -S --cuda-device-only $unit -o /tmp/tb_fe_$name/$stem.s 2>/dev/null
grep -A30 "amdhsa_kernel _ZN12_GLOBAL__N_122fast_tile_tiled_kernelILb1EEE" /tmp/tb_fe_$name/$stem.s | grep -E "group_segment|next_free_vgpr|scratch" | tr -s '\t\n' ' '; echo " <- $name"
