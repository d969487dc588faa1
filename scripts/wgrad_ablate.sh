# timing ablations of the filter-gradient kernels (SG_X6_ABLATE: 1 no loads, 2 no store / barriers, 4 no fragment reads + MFMAs,
# 8 no fragment reads: MFMAs on stale registers)
mkdir -p gpurun_out/$1
out=$_/ablate.txt   # ($_: the directory just made)
for a in 0 3 11; do
  echo "== SG_X6_ABLATE=$a" >> $out
  SG_X6_ABLATE=$a python scripts/wgrad_planes_bench.py 2>&1 | grep -E "HxW|2048   256 3|64x64    512|128x128   256" >> $out
done
cat gpurun_out/$1/ablate.txt
