#!/bin/bash
# copy what tools/collect_round.sh a / b / c left in $OUT/ to profiles/ under the round's names: bash tools/copy_profiles.sh r03
OUT=${OUT:-out}   # the folder tools/collect_round.sh wrote to
r=${1:-r03}
c() { [ -s "$1" ] && cp "$1" "$2"; }
c $OUT/bench_pallas.json profiles/${r}_bench_poseidon_k16_pallas.json
c $OUT/final_kernel_stats.csv profiles/${r}_bench_poseidon_k16_pallas_kernel_stats.csv
c $OUT/final_bench.json profiles/${r}_bench_poseidon_k16_pallas_under_rocprof.json
c $OUT/msm20_kernel_stats.csv profiles/${r}_msm_2e20_pallas_kernel_stats.csv
c $OUT/msm20_bench.json profiles/${r}_msm_2e20_pallas_under_rocprof.json
c $OUT/microbench_tail.txt profiles/${r}_microbench_tail.txt
c $OUT/bench_bn254.json profiles/${r}_bench_poseidon_k16_bn254.json
c $OUT/cfg.jsonl profiles/${r}_configs_3_4_5.jsonl
c $OUT/proof_gen.json profiles/${r}_proof_gen_k16.json
c $OUT/proof_trace.txt profiles/${r}_proof_trace_k16.txt
c $OUT/proof_gen_two_contexts.json profiles/${r}_proof_gen_k16_two_contexts_one_gpu.json
c $OUT/all_circuits_k16.json profiles/${r}_proof_all_circuits_k16.json
c $OUT/bench_gpus2.json profiles/${r}_bench_gpus2_shared_gpu_rehearsal.json
c $OUT/kc_proof_kernel_stats.csv profiles/${r}_proof_poseidon_k16_bn254_kernel_stats_key_cached.csv
c $OUT/nokc_proof_kernel_stats.csv profiles/${r}_proof_poseidon_k16_bn254_kernel_stats.csv
c $OUT/kc_pstats.txt profiles/${r}_proof_poseidon_k16_bn254_per_proof_key_cached.txt
c $OUT/pmc_traffic.json profiles/pmc_traffic.json
c $OUT/ntt_times.txt profiles/${r}_ntt_times.txt
c $OUT/sweep_tmax.txt profiles/${r}_sweep_entries_per_thread.txt
c $OUT/sweep_s2.txt profiles/${r}_sweep_two_level_sort.txt
c $OUT/sweep_sort2.txt profiles/${r}_sweep_two_level_sort_at_k16.txt
c $OUT/sq_ntt19.txt profiles/${r}_sq_counters_ntt_7x2e19.txt
true
