# One rocprofv3 counter pass (SQ counters only, with --kernel-trace; no other trace domains) over one bench step:
# matrix-pipe busy fraction per kernel family at the clock the kernels actually ran at.
#   OUT_DIR=<dir> bash scripts/profile_mfma_busy.sh      (output directory, default gpu_out/)
cd "$(dirname "$0")/.."; export TMPDIR=/tmp; mkdir -p "${OUT_DIR:-gpu_out}"; O=$(cd "${OUT_DIR:-gpu_out}" && pwd)
rm -rf $O/pmc_busy
(cd /tmp && timeout 240 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_LDS SQ_WAIT_ANY \
   -d "$O/pmc_busy" -o r1 --output-format csv -- python "$OLDPWD/bench.py" --full --steps 1 --warmup 1 --no-cpu-baseline > "$O/pmc_busy.log" 2>&1)
python tools/pmc_mfma_busy.py $O/pmc_busy > $O/pmc_mfma_busy.txt 2>&1
cat $O/pmc_mfma_busy.txt
head -1 $(find $O/pmc_busy -name '*counter_collection.csv' | head -1) > $O/pmc_busy_header.txt
find $O/pmc_busy -name '*.csv' -size +8M -delete
