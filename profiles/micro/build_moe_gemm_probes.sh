#!/bin/bash
# K25: which token tile should gq_linear_packed_experts take when the host does not know the counts?  The shipped source carries
# no probe switch, so the two variants are made by editing a copy of its one rule line: libgq_moe_wide.so always takes the
# 256-token tile (where the type has it), libgq_moe_narrow.so always the 128-token one.  Same results by construction (the bits do
# not depend on the tile).  Builds profiles/micro/_build/libgq_moe_{wide,narrow}.so (git-ignored; they travel to the GPU box) from
# the objects of a finished `make -C gptq-gguf-toolkit_amd/csrc`; run:
#   GQ_SO_PATH=$PWD/profiles/micro/_build/libgq_moe_wide.so python profiles/moe_prefill_rate.py --only grouped --tag wide --out FILE
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
S=$R/gptq-gguf-toolkit_amd/csrc
B=$R/profiles/micro/_build
mkdir -p $B
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wno-unused-function"
OBJS=$(ls $S/*.o $S/*/*.o | grep -v gq_moe_gemm.o)
for V in wide narrow; do
  python3 - "$S/qgemm/gq_moe_gemm.hip" "$S/qgemm/gq_moe_gemm_probe_$V.hip" "$V" <<'PY'
import sys
src, dst, v = sys.argv[1:]
s = open(src).read()
old = "P >= 128 * E;"
assert s.count(old) == 1
open(dst, "w").write(s.replace(old, "true;" if v == "wide" else "false;"))
PY
  /opt/rocm/bin/hipcc $FLAGS -c $S/qgemm/gq_moe_gemm_probe_$V.hip -o $B/gq_moe_gemm_$V.o
  rm -f $S/qgemm/gq_moe_gemm_probe_$V.hip   # (the copy lies beside the source for its relative includes, and only while it compiles)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $B/libgq_moe_$V.so $OBJS $B/gq_moe_gemm_$V.o
done
ls -la $B/libgq_moe_*.so
