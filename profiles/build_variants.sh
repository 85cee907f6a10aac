#!/bin/bash
# Build A/B variants of libivfpq.so (compile-time experiment switches) into lib/var/<name>/.
# Usage: build_variants.sh name:"-DFOO=1 -DBAR=2" ...   ; select one at run time with IVFPQ_LIB=<path>.
# Without arguments: the variants that are kept in the tree behind a macro, so that they are compiled somewhere:
#   fourpass  -DSCAN_LEAN_PASSES=4  (four-pass k_scan_lean, profiles/scan_four_pass.md)
#   onepass   -DSCAN_LEAN_SPLIT=0   (one-pass k_scan_lean, profiles/scan_split_lut.md)
#   nofill    -DPLAN_FILL_LEAD=0    (work items of one kind only, profiles/plan_fill_lead.md)
#   noitembound -DSCAN_ITEM_BOUND=0 (tau_q from the per-wave k-th keys only, profiles/scan_item_bound.md)
#   lutlinear -DSCAN_LUT_DWORD=0 -DSCAN_LUT_ROTATE=0 (k_scan_lean's table build by row vectors, stores in the order
#             c = 0..3: the scan before profiles/lut_store_banks.md)
#   lutrotate -DSCAN_LUT_DWORD=0 -DSCAN_LUT_ROTATE=1 (row vectors, stores rotated by the lane; same note)
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
C=$R/chameleon-rag-acceleration_amd/csrc
L=$R/chameleon-rag-acceleration_amd/lib
F="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=off -I$R/include -I$C"
[ $# -gt 0 ] || set -- "fourpass:-DSCAN_LEAN_PASSES=4" "onepass:-DSCAN_LEAN_SPLIT=0" "nofill:-DPLAN_FILL_LEAD=0" \
  "noitembound:-DSCAN_ITEM_BOUND=0" \
  "lutlinear:-DSCAN_LUT_DWORD=0 -DSCAN_LUT_ROTATE=0" "lutrotate:-DSCAN_LUT_DWORD=0 -DSCAN_LUT_ROTATE=1"
for spec in "$@"; do
  name=${spec%%:*}; defs=${spec#*:}
  O=$R/chameleon-rag-acceleration_amd/lib/var/$name
  mkdir -p "$O"
  /opt/rocm/bin/hipcc $F -mllvm -amdgpu-atomic-optimizer-strategy=None $defs -c -o "$O/k.o" "$C/ivfpq_kernels.hip" &
  /opt/rocm/bin/hipcc $F $defs -x hip -c -o "$O/i.o" "$C/ivfpq_index.cpp" &
  /opt/rocm/bin/hipcc $F $defs -c -o "$O/b.o" "$C/ivfpq_build.hip" &
  /opt/rocm/bin/hipcc $F $defs -c -o "$O/p.o" "$C/pq_flat.hip" &
  wait
  # the other indexes' objects do not depend on the switches: the default build's (run make first)
  rest=$(ls "$L"/*.o | grep -v -e /ivfpq_kernels.o -e /ivfpq_index.o -e /ivfpq_build.o -e /pq_flat.o)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$O/libivfpq.so" "$O/k.o" "$O/b.o" "$O/p.o" "$O/i.o" $rest
  rm -f "$O/k.o" "$O/i.o" "$O/b.o" "$O/p.o"
  echo "built $name ($defs)"
done
