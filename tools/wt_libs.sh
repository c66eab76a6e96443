#!/bin/bash
# Product-flavour libraries that differ only in L2D_WT_MASK (csrc/common.h: which kernel families write their output rows with
# write-through stores), for the same-box A/B of DESIGN.md section 9:
#   bash tools/wt_libs.sh            -> live2diff_amd/ablate/libl2d_wt<mask>.so for mask 0, every single family bit, and all bits  (CPU)
#   bash tools/wt_libs.sh "3 67"     -> ... and these masks as well
#   L2D_LIB=live2diff_amd/ablate/libl2d_wt64.so python bench.py ...                                                               (GPU box)
# Every touched file is compiled twice (mask 0 and its own bit); a mask's library is then only a different link of those objects.
set -e
cd "$(dirname "$0")/.."
C=live2diff_amd/csrc; O=live2diff_amd/ablate; mkdir -p $O
make -C $C -j8 2>&1 | tail -1
# family bit -> translation units
declare -A FILES=([1]="rowchain" [2]="rowgemm" [4]="wsgemm" [8]="igemm pconv" [16]="cconv" [32]="tattn_ring" [64]="norm")
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast -Wno-unused-result -Wno-unused-value -Xclang -target-feature -Xclang -packed-fp32-ops"
for bit in "${!FILES[@]}"; do
  for f in ${FILES[$bit]}; do
    for m in 0 $bit; do
      /opt/rocm/bin/hipcc $FLAGS -DL2D_WT_MASK=$m -c $C/$f.hip -o $O/${f}_wt$m.o 2>&1 | grep -v "not a recognized\|hip-link" &
    done
  done
done; wait
ALL=""; for bit in "${!FILES[@]}"; do ALL="$ALL ${FILES[$bit]}"; done
REST=$(ls $C/*.o | grep -v probes); for f in $ALL; do REST=$(echo "$REST" | grep -v "/$f.o"); done
for mask in 0 1 2 4 8 16 32 64 127 $1; do
  objs=""
  for bit in "${!FILES[@]}"; do
    for f in ${FILES[$bit]}; do
      if [ $((mask & bit)) -ne 0 ]; then objs="$objs $O/${f}_wt$bit.o"; else objs="$objs $O/${f}_wt0.o"; fi
    done
  done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $O/libl2d_wt$mask.so $REST $objs
done
rm -f $O/*_wt*.o; ls -la $O
