// h2_tune.hpp -- knobs of the tuning sweeps (tools/sweep_*.sh; results in DESIGN.md section 4).  They exist only in a
// build made with -DH2_TUNING (H2_BUILD_TUNING=1 python -m halo2_prover_amd.build --force): the product library never
// reads its configuration from the environment.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace h2 {
inline int tune_int(const char* name, int fallback) {
#ifdef H2_TUNING
  if (const char* v = getenv(name)) return atoi(v);
#else
  (void)name;
#endif
  return fallback;
}

// Proofs that h2_generate_proofs runs in lockstep (h2_prove.hpp); a larger batch is cut into groups of this many.
// Budget: 4 GiB of device memory for a group's columns at k = 16.  The widest circuit of the product surface (Poseidon:
// 4 advice, 1 instance and 2 product columns, extended domain 2^19 = 16 MiB a column) holds per proof 112 MiB of
// extended columns, 16 MiB of quotient and 28 MiB of Lagrange and coefficient columns; the extended transforms' second
// buffer adds up to 5 x 16 MiB per proof: 16 proofs come to 3.7 GiB.
// The budget is k = 16's: a group's columns double with every step of k, so above PROVE_GROUP_K the prover halves the group
// per step (create_proofs: 8 proofs at k = 17, 4 at 18, one from k = 20), and the 4 GiB hold at every k.
constexpr size_t PROVE_GROUP = 16;

// Terms below which the table-free MSM (h2_msm_points*, h2_msm_points.hpp) takes msm_small_kernel's double-and-add route
// instead of buckets: the smallest n of the sweep n = 8 ... 8192 from which the bucket route's median is lower
// (profiles/msm_points_crossover.txt, tools/msm_points_bench.py --crossover).  The bucket route is lower at EVERY swept
// n, 8 included (~0.9 ms against 1.3 - 1.6: both are one chain of ~255 doublings, and the double-and-add route also
// carries its additions on that chain), so the constant is the sweep's first size and only n < 8 is left to that route.
constexpr size_t MSM_POINTS_SMALL_MAX = 8;
constexpr uint32_t PROVE_GROUP_K = 16;

// Largest log n at which the group FFT (h2_group_fft.hpp) runs its stages four lanes per butterfly; above it, one lane.
// Where the two forms cross (tools/gfft_times.py with the form forced, profiles/gfft_times.txt):
// at 2^16 four lanes take 17.2 ms against 18.6 (BN254; Pallas 15.4 / 16.2), at 2^17 34.5 against 20.2 (31.2 / 17.6).
// The value derived before measuring was 17 (4 lanes x n/2 butterflies <= 1024 SIMDs x 4 waves x 64 lanes); both forms
// hold two waves a SIMD, not four (their registers), which moves the crossing one size down.
constexpr uint32_t GFFT_QUAD_MAX_LOG_N = 16;
}  // namespace h2
