# MFMA shape and deferred-MFMA count of the three-plane (exact route) product kernel, timed on one box; prints one line per build:
#   bash scripts/probes/shape3_variants.sh "SHAPE DEFER" ...     (defaults below)
# SHAPE: MDG_I8_SHAPE3, 16 (v_mfma_i32_16x16x64_i8, DEFER 0 .. 24 of its 72 MFMAs per stage) or 32 (v_mfma_i32_32x32x32_i8, of 36).
# Leaves the library built with the last variant: run make again afterwards.
[ $# -eq 0 ] && set -- "32 8" "16 0" "16 4" "16 8" "16 12" "16 16" "16 20" "16 24"
for v in "$@"; do
  set -- $v
  touch modegpt_amd/csrc/cov_i8_product.hip
  make -C modegpt_amd/csrc CXXFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-unused-variable -DMDG_I8_SHAPE3=$1 -DMDG_I8_DEFER3=$2" > /dev/null 2>&1 || { echo "build failed: $v"; exit 1; }
  echo "== shape $1, deferred $2"
  timeout -k 10 200 python3 scripts/probes/exact_route_timing.py 14336 32768 gaussian exact 2>&1 | grep "exact=True" | cut -c1-130 || exit 1
done
