# One collection run of the evidence under profiles/ (round tag = $1, default r06).  Run on a machine with an MI355X:
#   bash tools/run_profiles.sh r06      then   python tools/profile_summary.py r06      (raw output under out/)
# The stats pass and every PMC pass are separate rocprofv3 runs (counters are never combined with trace domains).
TAG=${1:-r06}
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R"
export TMPDIR=/tmp
mkdir -p out/prof
# the stats pass profiles the DEFAULT bench (two half-launches per step); the counter passes run one launch per step (--streams 1):
# launches 0-4 of the process are then cold solves of the 1024-agent batch, the rest receding-horizon steps of all 1024 agents
B1="python $R/bench.py --full --no-cpu --no-extras --no-parity"
B="python $R/bench.py --full --streams 1 --no-cpu --no-extras --no-parity"
( cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $R/out/prof/stats -- $B1 > $R/out/prof/bench_stats.json 2> $R/out/prof/stats.err )
( cd /tmp && rocprofv3 --pmc FETCH_SIZE --output-format csv -d $R/out/prof/fetch -- $B --steps 5 --warmup 1 > /dev/null 2> $R/out/prof/fetch.err )
# the L2 pass (hits, misses, read requests to the fabric) is a run of its own like every other counter set; once one launch per step,
# once in the default three-launch form (under --pmc the launches of the sub-batches run one after the other); the plain bench line,
# so that every solve-kernel launch of the process is a cold solve or a step of the headline batch
L2="python $R/bench.py --gpus 1 --steps 5 --warmup 1"
( cd /tmp && rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum TCC_REQ_sum --output-format csv -d $R/out/prof/l2 -- $L2 --streams 1 > /dev/null 2> $R/out/prof/l2.err )
( cd /tmp && rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum TCC_REQ_sum --output-format csv -d $R/out/prof/l2_default -- $L2 > /dev/null 2> $R/out/prof/l2_default.err )
python $R/tools/pmc_per_launch.py $R/out/prof/l2 > $R/out/${TAG}_pmc_l2.txt 2>&1; python $R/tools/pmc_per_launch.py $R/out/prof/l2_default >> $R/out/${TAG}_pmc_l2.txt 2>&1
( cd /tmp && rocprofv3 --pmc WRITE_SIZE --output-format csv -d $R/out/prof/write -- $B --steps 5 --warmup 1 > /dev/null 2> $R/out/prof/write.err )
( cd /tmp && rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F64 --output-format csv -d $R/out/prof/mfma -- $B --steps 5 --warmup 1 > /dev/null 2> $R/out/prof/mfma.err )
( cd /tmp && rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS --output-format csv -d $R/out/prof/lds -- $B --steps 5 --warmup 1 > /dev/null 2> $R/out/prof/lds.err )
( cd /tmp && rocprofv3 --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAVE_CYCLES --output-format csv -d $R/out/prof/wait -- $B --steps 5 --warmup 1 > /dev/null 2> $R/out/prof/wait.err )
python tools/phase_profile.py 1024 > out/${TAG}_phase_cycles_cold.json 2> out/phase.err
python tools/phase_profile.py 1024 mpc > out/${TAG}_phase_cycles_mpc.json 2>> out/phase.err
( cd /tmp && rocprofv3 --pmc SQ_WAIT_INST_LDS SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_WAVE_CYCLES SQ_INSTS_SALU SQ_INSTS_VALU SQ_INST_CYCLES_SALU SQ_IFETCH --output-format csv -d $R/out/prof/issue1 -- $B --steps 5 --warmup 1 > /dev/null 2> $R/out/prof/issue1.err )
( cd /tmp && rocprofv3 --pmc SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQ_ACTIVE_INST_ANY SQ_INSTS_SMEM SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_BUSY_CYCLES --output-format csv -d $R/out/prof/issue2 -- $B --steps 5 --warmup 1 > /dev/null 2> $R/out/prof/issue2.err )
( cd /tmp && rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_WAVES SQ_BUSY_CYCLES --output-format csv -d $R/out/prof/occ -- $B --steps 5 --warmup 1 > /dev/null 2> $R/out/prof/occ.err )
python bench.py --full --streams 1 --no-cpu --no-extras > out/${TAG}_bench_n1_one_launch_per_step.json 2> out/bench_1s.err
python bench.py --full --scaling strong --no-cpu --no-extras > out/${TAG}_bench_n1_strong.json 2> out/bench_strong.err
python bench.py --full --agents 4096 --no-cpu --no-extras > out/${TAG}_bench_n1_4096agents.json 2> out/bench_4096.err
python bench.py --full --agents 256 --no-cpu --no-extras > out/${TAG}_bench_n1_256agents.json 2> out/bench_256.err
python bench.py --full --tol 1e-6 --no-cpu --no-extras > out/${TAG}_bench_n1_tol1e-6.json 2> out/bench_tol.err
python bench.py --full --ipopt-defaults --no-cpu --no-extras > out/${TAG}_bench_n1_ipopt_default_tolerances.json 2> out/bench_ipd.err
python bench.py --workload quadrotor --agents 4096 --steps 5 --warmup 2 > out/${TAG}_bench_quadrotor_4096.json 2> out/bench_quadrotor4096.err
python bench.py --workload holonomic3d --agents 8192 --steps 3 --warmup 1 > out/${TAG}_bench_holonomic3d_8192.json 2> out/bench_h3d8192.err
python bench.py --workload formation --steps 50 --warmup 5 > out/${TAG}_bench_formation_n1.json 2> out/bench_formation.err
python bench.py --workload rendezvous --steps 50 --warmup 5 > out/${TAG}_bench_rendezvous.json 2> out/bench_rendezvous.err
python bench.py --workload quadrotor --steps 5 --warmup 2 > out/${TAG}_bench_quadrotor.json 2> out/bench_quadrotor.err
python bench.py --workload holonomic3d --steps 3 --warmup 1 > out/${TAG}_bench_holonomic3d.json 2> out/bench_holonomic3d.err
python tools/cpu_pool_sweep.py > out/${TAG}_cpu_pool_sweep.txt 2>&1
python bench.py --full > out/${TAG}_bench_n1.json 2> out/bench_final.err
cp out/prof/bench_stats.json out/${TAG}_bench_n1_under_rocprof.json
python tools/profile_summary.py ${TAG} > out/${TAG}_profile_summary.txt 2>&1; mkdir -p out/profiles; python tools/profile_summary.py ${TAG} issue >> out/${TAG}_profile_summary.txt 2>&1
cp profiles/${TAG}_kernel_stats.csv profiles/${TAG}_pmc_*.json out/profiles/ 2>/dev/null
tail -30 out/${TAG}_profile_summary.txt
ls out/prof/*/ | head -30
