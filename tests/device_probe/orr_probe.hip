// orr_probe.hip -- TEST-ONLY probe of the env kernels' device primitives (tests/probe_lib.py, tests/test_gpu_device_primitives.py).
//
// Not part of libopenroborl_hip.so: it includes the env kernels' header, instantiates no step or reset kernel, and wraps the LEAF device
// helpers of orr_device.h / orr_physics.h / orr_task.h in a small kernel each:
//   extern "C" int orrp_<name>(const void* in, void* out, int n, void* stream)
// Probed here: joint_sincos, atan2_bf, asin_bf, map_pi, q_norm_angle, euler_from_quat, qheading, qslerp, q_to_mat, qrot, pick4; row_sum16,
// bcast_lane, dpp_bcast_max0, dpp_contact_triplet, part_suffix_sum (+ _inplace, _first_moment), zero_in_lane; chol6 / chol6_solve and
// chol6_pk / chol6_solve_pk; philox_block, time_limit.  Probed by the siblings: normal_pair (orr_probe_noise.hip); the two solver stages
// built from these leaves, delassus_columns and pgs_sweeps, which take their operands in registers (orr_probe_solver.hip).
// NOT probed HERE: row_setup_bank_a / row_setup_limit, row_response and leg_dynamics read and write the per-robot LDS image (Shared) and
// need KParams and the device tables, so they cannot be driven with chosen register inputs.  Their outputs are read stage by stage
// through the -DORR_STAGE_DUMP build of the library itself (orr_stage_dump_kernel, csrc/orr_env_kernels.h) and compared with float64
// by tests/test_gpu_substep_stages.py; the sub-step parity tests (tests/test_gpu_parity.py, tests/test_gpu_substep_paths.py) see them
// through a whole sub-step.
// `in` / `out` are DEVICE pointers to n records of the helper's arguments / results (array of records, 4-byte words; the layouts
// are listed at each entry point and mirrored by tests/probe_lib.py: SPECS).  Returns 0, or -1 for a bad n, or the hipError_t of the
// launch.  One lane serves one record; every kernel checks its bounds and has no data-dependent loop.
// The cross-lane (DPP) helpers need every lane of a wave active: their entry points take whole waves only (n a multiple of 64, at
// least two blocks), and record i sits in lane i & 63, i.e. robot (i >> 4) & 3 of its wave, lane i & 15 of that robot.
#include "orr_env_kernels.h"

namespace {

// ---- one lane, one record ------------------------------------------------------------------------------------------------------
template <int NIN, int NOUT, typename F>
__global__ __launch_bounds__(64) void probe_kernel(const float* __restrict__ in, float* __restrict__ out, int n, F f) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n) return;
  float a[NIN], o[NOUT];
#pragma unroll
  for (int k = 0; k < NIN; k++) a[k] = in[(size_t)i * NIN + k];
  f(a, o, i);
#pragma unroll
  for (int k = 0; k < NOUT; k++) out[(size_t)i * NOUT + k] = o[k];
}
// ---- whole waves: no lane leaves before the helper ran (n is a multiple of 64: the entry point checked it) -----------------------
template <int NIN, int NOUT, typename F>
__global__ __launch_bounds__(64) void probe_wave_kernel(const float* __restrict__ in, float* __restrict__ out, int n, F f) {
  if (((int)blockIdx.x + 1) * 64 > n) return;   // wave-uniform
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  float a[NIN], o[NOUT];
#pragma unroll
  for (int k = 0; k < NIN; k++) a[k] = in[(size_t)i * NIN + k];
  f(a, o, i);
#pragma unroll
  for (int k = 0; k < NOUT; k++) out[(size_t)i * NOUT + k] = o[k];
}

template <int NIN, int NOUT, typename F>
int launch(const void* in, void* out, int n, void* stream, F f) {
  if (n <= 0 || !in || !out) return -1;
  hipLaunchKernelGGL((probe_kernel<NIN, NOUT, F>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const float*)in,
                     (float*)out, n, f);
  return (int)hipGetLastError();
}
template <int NIN, int NOUT, typename F>
int launch_wave(const void* in, void* out, int n, void* stream, F f) {
  if (n < 128 || n % 64 != 0 || !in || !out) return -1;
  hipLaunchKernelGGL((probe_wave_kernel<NIN, NOUT, F>), dim3((unsigned)(n / 64)), dim3(64), 0, (hipStream_t)stream, (const float*)in,
                     (float*)out, n, f);
  return (int)hipGetLastError();
}

template <int A, int B, typename F>
__device__ __forceinline__ void for_range(F&& f) {
  if constexpr (A < B) {
    f(std::integral_constant<int, A>{});
    for_range<A + 1, B>(f);
  }
}

}  // namespace

#define PROBE(name, NIN, NOUT, ...)                                                                  \
  extern "C" int orrp_##name(const void* in, void* out, int n, void* stream) {                       \
    return launch<NIN, NOUT>(in, out, n, stream, [] __device__(const float* a, float* o, int i) __VA_ARGS__); \
  }
#define PROBE_WAVE(name, NIN, NOUT, ...)                                                             \
  extern "C" int orrp_##name(const void* in, void* out, int n, void* stream) {                       \
    return launch_wave<NIN, NOUT>(in, out, n, stream, [] __device__(const float* a, float* o, int i) __VA_ARGS__); \
  }

// ================================================================================================
// branch-free math
// ================================================================================================
PROBE(joint_sincos, 1, 2, { joint_sincos(a[0], &o[0], &o[1]); })              // a -> (sin, cos)
PROBE(atan2_bf, 2, 1, { o[0] = atan2_bf(a[0], a[1]); })                        // (y, x)
PROBE(asin_bf, 1, 1, { o[0] = asin_bf(a[0]); })
PROBE(map_pi, 1, 1, { o[0] = map_pi(a[0]); })
PROBE(q_norm_angle, 4, 1, { o[0] = q_norm_angle(a); })                         // xyzw
PROBE(euler_from_quat, 4, 3, { euler_from_quat(a, o); })                       // xyzw -> roll pitch yaw
PROBE(qheading, 4, 1, { o[0] = qheading(a); })
PROBE(qslerp, 9, 4, { qslerp(&a[0], &a[4], a[8], o); })                        // (a, b, f)
PROBE(q_to_mat, 4, 9, { q_to_mat(a, o); })
PROBE(qrot, 7, 3, { qrot(&a[0], &a[3], o); })                                  // (p, q)
PROBE(pick4, 4, 1, { o[0] = pick4(i, a[0], a[1], a[2], a[3]); })               // lane = record index

// ================================================================================================
// cross-lane (DPP) helpers: whole waves
// ================================================================================================
PROBE_WAVE(row_sum16, 1, 1, { o[0] = row_sum16(a[0]); })
PROBE_WAVE(bcast_lane, 1, 16, {                                                // out[R] = bcast_lane<R>, R = 0..15
  const float x = a[0];
  const int sub = (i >> 4) & 3;
  for_range<0, 16>([&](auto rc) __attribute__((always_inline)) { o[decltype(rc)::value] = bcast_lane<decltype(rc)::value>(x, sub); });
})
PROBE_WAVE(dpp_bcast_max0, 1, 12, {                                            // out[R - 4] = dpp_bcast_max0<R>, R = 4..15 (the sweeps' slots)
  const float x = a[0];
  float zero;
  asm("v_mov_b32 %0, 0" : "=v"(zero));   // a VGPR operand, as in pgs_sweeps
  for_range<4, 16>([&](auto rc) __attribute__((always_inline)) { o[decltype(rc)::value - 4] = dpp_bcast_max0<decltype(rc)::value>(x, zero); });
})
// in: rr[3], c00 c01 c02 c10 c11 c12 c20 c21 c22, wa[6], wq[3]; out[3 g + (x, y, z)] = dpp_contact_triplet<4 + g>
PROBE_WAVE(dpp_contact_triplet, 21, 12, {
  for_range<0, 4>([&](auto gc) __attribute__((always_inline)) {
    constexpr int g = decltype(gc)::value;
    dpp_contact_triplet<4 + g>(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15], a[16],
                               a[17], a[18], a[19], a[20], o[3 * g], o[3 * g + 1], o[3 * g + 2]);
  });
})
PROBE_WAVE(part_suffix_sum, 1, 1, { o[0] = part_suffix_sum(a[0]); })
PROBE_WAVE(part_suffix_sum_inplace, 6, 6, {
  float v[6] = {a[0], a[1], a[2], a[3], a[4], a[5]};
  part_suffix_sum_inplace(v);
  for (int k = 0; k < 6; k++) o[k] = v[k];
})
// in: m, c[3], h[3] (h = the lane's ROUNDED m c, as leg_dynamics holds it); out: h[3], m
PROBE_WAVE(part_suffix_sum_first_moment_m0, 7, 4, {
  float m = a[0];
  const float c[3] = {a[1], a[2], a[3]};
  float h[3] = {a[4], a[5], a[6]};
  part_suffix_sum_first_moment<false>(m, c, h);
  o[0] = h[0]; o[1] = h[1]; o[2] = h[2]; o[3] = m;
})
PROBE_WAVE(part_suffix_sum_first_moment_m1, 7, 4, {
  float m = a[0];
  const float c[3] = {a[1], a[2], a[3]};
  float h[3] = {a[4], a[5], a[6]};
  part_suffix_sum_first_moment<true>(m, c, h);
  o[0] = h[0]; o[1] = h[1]; o[2] = h[2]; o[3] = m;
})
PROBE_WAVE(zero_in_lane, 1, 16, {                                              // out[K] = zero_in_lane<K>, K = 0..15
  const float x = a[0];
  const int lane = i & 15;
  for_range<0, 16>([&](auto kc) __attribute__((always_inline)) { o[decltype(kc)::value] = zero_in_lane<decltype(kc)::value>(x, lane); });
})

// ================================================================================================
// 6x6 Cholesky: in = A (36, row-major, full) + b (6); out = x (6) + 1 / diagonal (6)
// ================================================================================================
PROBE(chol6, 42, 12, {
  float L[21], idg[6];
  chol6(a, L, idg);
  chol6_solve(L, idg, &a[36], o);
  for (int k = 0; k < 6; k++) o[6 + k] = idg[k];
})
// the argument layout of leg_dynamics' call: the lower triangle by columns, rows (2,3) and (4,5) paired
#define A_(r, c) a[(r) * 6 + (c)]
PROBE(chol6_pk, 42, 12, {
  Chol6Pk F;
  chol6_pk(A_(0, 0), A_(1, 1), A_(3, 3), A_(5, 5), A_(1, 0), pk2{A_(2, 2), A_(3, 2)}, pk2{A_(4, 4), A_(5, 4)},
           pk2{A_(2, 0), A_(3, 0)}, pk2{A_(4, 0), A_(5, 0)}, pk2{A_(2, 1), A_(3, 1)}, pk2{A_(4, 1), A_(5, 1)},
           pk2{A_(4, 2), A_(5, 2)}, pk2{A_(4, 3), A_(5, 3)}, F);
  chol6_solve_pk(F, a[36], a[37], pk2{a[38], a[39]}, pk2{a[40], a[41]}, o);
  for (int k = 0; k < 6; k++) o[6 + k] = F.idg[k];
})
#undef A_

// ================================================================================================
// counter-based RNG and step limit (integer records)
// ================================================================================================
namespace {
__global__ __launch_bounds__(64) void probe_philox(const uint32_t* __restrict__ in, float* __restrict__ out, int n) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n) return;
  const uint32_t* r = in + (size_t)i * 6;
  float u[4];
  philox_block((unsigned long long)r[0] | ((unsigned long long)r[1] << 32), r[2], r[3], r[4], u);
  for (int k = 0; k < 4; k++) out[(size_t)i * 4 + k] = u[k];
}
__global__ __launch_bounds__(64) void probe_time_limit(const orr_config* __restrict__ cfg, const long long* __restrict__ total,
                                                       int* __restrict__ out, int n) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n) return;
  out[i] = time_limit(*cfg, total[i]);
}
}  // namespace
// in: n records of 6 words (seed low, seed high, robot, episode, block, unused); out: 4 floats
extern "C" int orrp_philox_block(const void* in, void* out, int n, void* stream) {
  if (n <= 0 || !in || !out) return -1;
  hipLaunchKernelGGL(probe_philox, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const uint32_t*)in, (float*)out, n);
  return (int)hipGetLastError();
}
// in: one orr_config, padded to a multiple of 8 bytes, then n int64 totals; out: n int32
extern "C" int orrp_time_limit(const void* in, void* out, int n, void* stream) {
  if (n <= 0 || !in || !out) return -1;
  const size_t off = (sizeof(orr_config) + 7) & ~(size_t)7;
  hipLaunchKernelGGL(probe_time_limit, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const orr_config*)in,
                     (const long long*)((const char*)in + off), (int*)out, n);
  return (int)hipGetLastError();
}
extern "C" int orrp_sizeof_config(void) { return (int)sizeof(orr_config); }
