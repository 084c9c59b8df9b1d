#!/bin/bash
# Developer tool: where the headline solve kernel (ipm_solve_kernel<WS_JAC_HV, true, false>, unit omgx_inst_solve_wave.hip) touches
# scratch memory -- line numbers of the scratch instructions within the kernel's disassembly, and the kernel's length.
#   spill_sites.sh [OBJECT]     default: omg-tools_amd/csrc/build/omgx_inst_solve_wave.o (make -C omg-tools_amd/csrc build/omgx_inst_solve_wave.o)
T=/tmp/hl_dis; mkdir -p $T
/opt/rocm/lib/llvm/bin/llvm-objcopy -O binary --only-section=.hip_fatbin ${1:-$(dirname $0)/../omg-tools_amd/csrc/build/omgx_inst_solve_wave.o} $T/fat.bin
/opt/rocm/lib/llvm/bin/clang-offload-bundler --unbundle --type=o --input=$T/fat.bin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$T/co.o
K=$(/opt/rocm/lib/llvm/bin/llvm-readelf -sW $T/co.o | grep -o "_Z16ipm_solve_kernelILi5ELb1ELb0ELb0ELb0E[A-Za-z0-9_]*" | grep -v kd | head -1)
/opt/rocm/lib/llvm/bin/llvm-objdump -d --mcpu=gfx950 --disassemble-symbols=$K $T/co.o > $T/solve.s
echo "kernel lines: $(wc -l < $T/solve.s); scratch ops at: $(grep -n 'scratch_store\|scratch_load' $T/solve.s | awk -F: '{print $1}' | tr '\n' ' ')"
echo "v_writelane $(grep -c v_writelane $T/solve.s) v_readlane $(grep -c v_readlane $T/solve.s) s_barrier $(grep -c s_barrier $T/solve.s)"
