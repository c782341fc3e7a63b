#!/bin/bash
# Run on the GPU box:  bash tools/profile_bench.sh <tag>     (e.g. r01)
# 1. rocprofv3 kernel trace of the bench.py --full command              -> $OUT/prof_<tag>/
# 2. separate PMC passes (FETCH_SIZE, WRITE_SIZE) of a short bench run  -> $OUT/pmc_<tag>_{rd,wr}/
# 3. markdown / json summaries                                          -> $OUT/<tag>_*.md|json  (copy into profiles/)
# $OUT is $PROFILE_OUT, by default profile_out/ in the repository root.
TAG=${1:-r01}
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=${PROFILE_OUT:-$R/profile_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_$TAG $OUT/pmc_${TAG}_rd $OUT/pmc_${TAG}_wr
rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o bench -- python3 $R/bench.py --full > $OUT/${TAG}_bench_default.log 2>&1
grep '^{' $OUT/${TAG}_bench_default.log | tail -1 > $OUT/${TAG}_bench_default.json
SHORT="--full --steps 3 --warmup 1 --no-cpu-baseline --sampler-steps 20"
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_${TAG}_rd -o rd -- python3 $R/bench.py $SHORT > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_${TAG}_wr -o wr -- python3 $R/bench.py $SHORT > /dev/null 2>&1
# 4. matrix-pipe evidence: MFMA busy cycles, effective clock (GRBM_GUI_ACTIVE / duration), issue stalls -- two SQ passes + GRBM
rm -rf $OUT/pmc_${TAG}_m1 $OUT/pmc_${TAG}_m2
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE -d $OUT/pmc_${TAG}_m1 -o m1 -- python3 $R/bench.py $SHORT > $OUT/${TAG}_pmc_m1.log 2>&1
rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_ANY GRBM_GUI_ACTIVE -d $OUT/pmc_${TAG}_m2 -o m2 -- python3 $R/bench.py $SHORT > $OUT/${TAG}_pmc_m2.log 2>&1
cd $R
HEADREV=$(git -C $R rev-parse --short HEAD 2>/dev/null || cat $R/.head_rev 2>/dev/null || echo snapshot)
python3 tools/rocpd_summary.py --mfma $(find $OUT/pmc_${TAG}_m1 $OUT/pmc_${TAG}_m2 -name "*.db") > $OUT/${TAG}_pmc_mfma.md
python3 tools/rocpd_summary.py --mfma-json $(find $OUT/pmc_${TAG}_m1 $OUT/pmc_${TAG}_m2 -name "*.db") > $OUT/${TAG}_pmc_mfma.json   # -> profiles/pmc_mfma.json (bench.py looks it up)
# per-dispatch view of the two epilogue-heavy training GEMMs (position 0 of EpiGNBwd = the K = 64 post_dense launch: epilogue only;
# position 0 of EpiGN<train> = layer 0 with K = 576 against K = 1536): VALU / MFMA instructions, busy cycles and durations per position
{
  echo "# per-dispatch counters of the GroupNorm training GEMMs, folded over the steps ($TAG)"
  python3 tools/rocpd_summary.py --dispatches "256x256,EpiGNBwd" 5 $(find $OUT/pmc_${TAG}_m1 $OUT/pmc_${TAG}_m2 -name "*.db")
  python3 tools/rocpd_summary.py --dispatches "256x256,EpiGN<train>" 5 $(find $OUT/pmc_${TAG}_m1 $OUT/pmc_${TAG}_m2 -name "*.db")
} > $OUT/${TAG}_epilogue_dispatches.md 2>&1
rm -rf $OUT/pmc_${TAG}_m1 $OUT/pmc_${TAG}_m2
python3 tools/rocpd_summary.py $(find $OUT/prof_$TAG -name "*.db" | head -1) > $OUT/${TAG}_bench_kernel_stats.md
python3 tools/rocpd_summary.py --pmc $(find $OUT/pmc_${TAG}_rd $OUT/pmc_${TAG}_wr -name "*.db") > $OUT/${TAG}_pmc_hbm_traffic.md
python3 tools/rocpd_summary.py --pmc-json $(find $OUT/pmc_${TAG}_rd $OUT/pmc_${TAG}_wr -name "*.db") > $OUT/${TAG}_pmc_hbm_traffic.json
# the raw rocpd databases are large: keep the summaries only
rm -rf $OUT/prof_$TAG $OUT/pmc_${TAG}_rd $OUT/pmc_${TAG}_wr
for f in $OUT/${TAG}_*.md; do sed -i "1s/^/commit $HEADREV (tools\/profile_bench.sh $TAG)\n\n/" $f; done
head -40 $OUT/${TAG}_epilogue_dispatches.md; head -30 $OUT/${TAG}_bench_kernel_stats.md; head -30 $OUT/${TAG}_pmc_mfma.md; head -24 $OUT/${TAG}_pmc_hbm_traffic.md; cat $OUT/${TAG}_bench_default.json
