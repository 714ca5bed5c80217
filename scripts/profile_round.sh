#!/bin/bash
# Everything the judged profile files come from, in one run on the GPU:
#   1. rocprofv3 --kernel-trace --stats of one bench step           -> profile_out/stats_<tag>.txt
#   2. rocprofv3 --pmc passes of the same command (HBM bytes; SQ)   -> profile_out/pmc_<tag>.json  (copied to profiles/r06_pmc.json,
#      which the bench line quotes: MFMA count, VALU per MFMA, stall fractions, HBM bytes per launch)
#   3. the bench.py --full line                                     -> profile_out/bench_<tag>.log
# usage: scripts/profile_round.sh <tag>          (copy the three files into profiles/ afterwards)
tag=$1
R=$(cd "$(dirname "$0")/.." && pwd)
O=$R/profile_out
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
CMD="python3 bench.py --steps 1 --warmup 0 --no-extras"
(cd $R && rocprofv3 --kernel-trace --stats -d $O/prof_${tag}/stats -o res -- $CMD) > $O/prof_${tag}_stats.log 2>&1
(cd $R && python3 scripts/rocpd_summary.py $(find $O/prof_${tag}/stats -name "*.db" | head -1) $O/stats_${tag}.txt; head -6 $O/stats_${tag}.txt)
i=0
for grp in "FETCH_SIZE" "WRITE_SIZE" "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR" \
           "SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_LDS_IDX_ACTIVE"; do
  i=$((i+1))
  (cd $R && rocprofv3 --pmc $grp --kernel-trace -d $O/prof_${tag}/pmc$i -o res -- $CMD) > $O/prof_${tag}_pmc$i.log 2>&1
done
cd $R
ver=$(python3 -c "import juqbox_jl_amd._lib as l; print(l.load().jq_version().decode())")
python3 scripts/make_traffic_json.py $O/pmc_${tag}.json --version "$ver" --samples ${JQ_BENCH_SAMPLES:-3072} --nsteps 32386 $(find $O/prof_${tag}/pmc* -name "*.db") && head -30 $O/pmc_${tag}.json
# the bench line last: it quotes the PMC figures of THIS build
cp $O/pmc_${tag}.json profiles/r06_pmc.json
python3 bench.py --full > $O/bench_${tag}.log 2> $O/bench_${tag}.err
tail -1 $O/bench_${tag}.log | cut -c1-1500
rm -rf $O/prof_${tag}      # (the rocpd databases are large; their summaries above are what is kept)
