#!/bin/bash
# Developer tool: register / spill / scratch numbers of the kernels of a libomgx build (code object notes), unit by unit.
#   kernel_resources.sh [BUILD_DIR | OBJECT] [REGEX]     default: the objects of omg-tools_amd/csrc/build (build/prof: the profiling build)
# Every line starts with the unit (object) that holds the kernel; exit status 1 when a kernel name occurs in more than one unit.
# One instance's numbers without the rest of the library (the headline instance ipm_solve_kernel<WS_JAC_HV, true, false> lives in
# omgx_inst_solve_wave.hip):  make -C omg-tools_amd/csrc build/omgx_inst_solve_wave.o && tools/kernel_resources.sh omg-tools_amd/csrc/build/omgx_inst_solve_wave.o
SRC=${1:-$(dirname $0)/../omg-tools_amd/csrc/build}
LLVM=/opt/rocm/lib/llvm/bin
T=$(mktemp -d)
case "$SRC" in *.so) echo "$SRC: a library holds one code-object bundle per unit and only the first would be read; give the build directory or an object" >&2; exit 2;; esac
if [ -d "$SRC" ]; then OBJS=$(ls "$SRC"/*.o); else OBJS=$SRC; fi
for O in $OBJS; do
  U=$(basename "$O" .o)
  $LLVM/llvm-objcopy -O binary --only-section=.hip_fatbin "$O" $T/fat.bin
  $LLVM/clang-offload-bundler --unbundle --type=o --input=$T/fat.bin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$T/co.o
  $LLVM/llvm-readelf --notes $T/co.o | grep -E "^ +(- )?\.(name|vgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):" | sed 's/^ *-\? *//' | awk '/^\.agpr_count/{if(rec)print rec; rec=""} {rec=rec" "$0} END{print rec}' | sed 's/_ZN4omgx//; s/_Z//' | sed -E "s/EvN4omgx.*Pyi//; s/ +/ /g; s/^ ?/$U /"
  ls -l $T/co.o | awk -v u=$U '{print u, "code object bytes:", $5}' >> $T/sizes
done > $T/all
grep -E "${2:-.}" $T/all | cut -c1-280
cat $T/sizes
DUP=$(sed -E 's/.*\.name: *([^ ]+).*/\1/' $T/all | sort | uniq -d)
rm -rf $T
if [ -n "$DUP" ]; then echo "kernels in more than one unit:"; echo "$DUP"; exit 1; fi
