#!/bin/bash
# rocprofv3 passes over bench.py on the GPU box (usage: scripts/profile_bench.sh <prefix> <outdir>):
# kernel trace + stats, then FETCH_SIZE, WRITE_SIZE and the SQ instruction counters in their own PMC passes
# (never combined with a trace domain).  Outputs under <outdir>/<prefix>_*; scripts/refresh_profiles.py
# copies the summaries into profiles/.  The passes whose lines need the roofline's counter pass, the machine calibration
# or the extras run bench.py --full.
P=$1
R=$PWD
O=$(realpath -m "${2:?usage: scripts/profile_bench.sh <prefix> <outdir>}")
export TMPDIR=/tmp
mkdir -p $O
cd /tmp
# kernel trace + stats of the timed launches (whole tile per launch).  --no-e2e: the untimed drop-in call at the end of
# the --full command launches the same kernel on 5 chunks of rows, which would mix into the per-kernel average; the
# --full command (with it and with the untimed extras except config 5: binary_search, discrete_sampling, the curved tile, c4)
# is traced as well, into ${P}_kte -- its per-kernel table is the rocprofv3 evidence for the ALG 0 / 1 instantiations
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${P}_kt -- \
    python $R/bench.py --full --no-cpu-baseline --no-e2e --no-extras > $O/${P}_kt_bench.json 2> $O/${P}_kt.err
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${P}_kte -- \
    python $R/bench.py --full --no-cpu-baseline --no-c5-extra > $O/${P}_kte_bench.json 2> $O/${P}_kte.err
timeout 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/${P}_fetch -- \
    python $R/bench.py --steps 2 > /dev/null 2> $O/${P}_fetch.err
timeout 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/${P}_write -- \
    python $R/bench.py --steps 2 > /dev/null 2> $O/${P}_write.err
timeout 600 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_WAVES SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_LDS --output-format csv -d $O/${P}_sq -- \
    python $R/bench.py --full --steps 2 --no-cpu-baseline --no-peaks --no-e2e --no-extras > $O/${P}_sq_bench.json 2> $O/${P}_sq.err
timeout 600 rocprofv3 --pmc GRBM_GUI_ACTIVE --output-format csv -d $O/${P}_grbm -- \
    python $R/bench.py --steps 2 > /dev/null 2> $O/${P}_grbm.err
# config 4 (shadow, 144 sun positions in one launch): kernel trace + stats, and the SQ counters of k_shadow_refill
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${P}_c4kt -- \
    python $R/bench.py --full --workload c4 > $O/${P}_c4kt_bench.json 2> $O/${P}_c4kt.err
timeout 600 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_WAVES SQ_INSTS_VMEM_RD --output-format csv -d $O/${P}_c4sq -- \
    python $R/bench.py --workload c4 --steps 2 > /dev/null 2> $O/${P}_c4sq.err
timeout 600 rocprofv3 --pmc GRBM_GUI_ACTIVE --output-format csv -d $O/${P}_c4grbm -- \
    python $R/bench.py --workload c4 --steps 2 > /dev/null 2> $O/${P}_c4grbm.err
# wait / busy split of the wave cycles, final kernels (two passes each: the SQ counters of one pass share 8 slots)
for W in "wb1:SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_BUSY_CYCLES" "wb2:SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_INSTS_VALU"; do
  tag=${W%%:*}; set=${W#*:}
  timeout 600 rocprofv3 --pmc $set --output-format csv -d $O/${P}_$tag -- \
      python $R/bench.py --steps 1 --warmup 1 > /dev/null 2> $O/${P}_$tag.err
  timeout 600 rocprofv3 --pmc $set --output-format csv -d $O/${P}_c4$tag -- \
      python $R/bench.py --workload c4 --steps 1 --warmup 0 > /dev/null 2> $O/${P}_c4$tag.err
done
cd $R
tail -1 $O/${P}_kt_bench.json | cut -c1-400
