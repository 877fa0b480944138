// orr_probe_noise.hip -- TEST-ONLY probe of normal_pair (csrc/orr_device.h), the device primitive of the task noise
// (tests/probe_noise_lib.py, tests/test_gpu_init_noise.py).  Not part of libopenroborl_hip.so; it includes the env kernels' header and
// instantiates no step or reset kernel.
//
//   extern "C" int orrp_normal_pair_sweep(const float* ub, int nub, int first, int count, double* out, unsigned long long* scratch, void* stream)
//   extern "C" int orrp_normal_pair(const void* in, void* out, int n, void* stream)      (n records (ua, ub) -> (z0, z1), one lane each)
//
// For each of the `nub` angles' uniforms ub[j] (device pointer, values m / 2^24) it evaluates normal_pair(ua, ub[j]) for the `count`
// radius uniforms ua = i / 2^24, i = first .. first + count - 1 (0 <= first, first + count <= 2^24), compares both results with the
// float64 definition and reduces on the device: out (device pointer, 2 * nub + 2 doubles, written whole) receives per angle
// [2 j] = max |z - z_float64| over the range and [2 j + 1] = the i of that maximum, then [2 nub] = how many of the 2 * nub * count
// results were not finite and [2 nub + 1] = count (a cross-check that the launch covered the range); scratch = nub + 2 zeroed 64-bit words.  The float64 definition is
// evaluated on the device too (its double-precision log / sqrt / sincos: there is no such thing in the env kernels, this file only);
// tests/test_gpu_init_noise.py checks that evaluation against numpy on a sample before it trusts the maximum.
// One workgroup per (angle, chunk of 2^16 ua); every access is bounds-checked; no data-dependent loop.
#include "orr_env_kernels.h"

namespace {
constexpr int kChunk = 1 << 16;

__global__ __launch_bounds__(256) void normal_pair_sweep_kernel(const float* __restrict__ ub, int nub, int first, int count, int chunks,
                                                                unsigned long long* __restrict__ packed, unsigned long long* __restrict__ tally) {
  const int j = (int)blockIdx.x / chunks, ch = (int)blockIdx.x % chunks;
  if (j >= nub) return;
  const float ubj = ub[j];
  const double phi = 6.283185307179586476925 * (double)ubj;
  const double c64 = cos(phi), s64 = sin(phi);
  double worst = 0.0;
  int worst_i = first;
  unsigned int bad = 0, done = 0;
  for (int k = (int)threadIdx.x; k < kChunk; k += 256) {
    const int off = ch * kChunk + k;
    if (off >= count) break;
    const int i = first + off;
    const float ua = (float)i * (1.0f / 16777216.0f);
    float z0, z1;
    orr::normal_pair(ua, ubj, &z0, &z1);
    const double r64 = sqrt(-2.0 * log1p(-(double)ua));
    const double e0 = fabs((double)z0 - r64 * c64), e1 = fabs((double)z1 - r64 * s64);
    const bool fin = fabsf(z0) < 1e30f && fabsf(z1) < 1e30f;
    bad += fin ? 0u : 1u;
    const double e = fin ? fmax(e0, e1) : 0.0;
    if (e > worst) { worst = e; worst_i = i; }
    done += j == 0 ? 1u : 0u;
  }
  // errors are >= 0: their bit patterns order like the numbers.  The top 40 bits of the error and the 24-bit index in one word
  const unsigned long long key = (((unsigned long long)__double_as_longlong(worst)) & ~0xFFFFFFull) | (unsigned long long)(worst_i & 0xFFFFFF);
  atomicMax(&packed[j], key);
  if (bad) atomicAdd(&tally[0], (unsigned long long)bad);
  if (done) atomicAdd(&tally[1], (unsigned long long)done);
}

__global__ void normal_pair_unpack_kernel(const unsigned long long* __restrict__ packed, const unsigned long long* __restrict__ tally, int nub,
                                          double* __restrict__ out) {
  const int j = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (j < nub) {
    out[2 * j] = __longlong_as_double((long long)(packed[j] & ~0xFFFFFFull));     // the error, rounded DOWN by at most 2^-28 of itself
    out[2 * j + 1] = (double)(packed[j] & 0xFFFFFFull);
  }
  if (j == 0) { out[2 * nub] = (double)tally[0]; out[2 * nub + 1] = (double)tally[1]; }
}
}  // namespace

// scratch_dev: nub + 2 64-bit words, zeroed by the caller
extern "C" int orrp_normal_pair_sweep(const float* ub_dev, int nub, int first, int count, double* out_dev, unsigned long long* scratch_dev, void* stream) {
  if (!ub_dev || !out_dev || !scratch_dev || nub < 1 || nub > 4096 || first < 0 || count < 1 || (long long)first + count > (1ll << 24)) return -1;
  const int chunks = (count + kChunk - 1) / kChunk;
  hipLaunchKernelGGL(normal_pair_sweep_kernel, dim3((unsigned)(nub * chunks)), dim3(256), 0, (hipStream_t)stream, ub_dev, nub, first, count, chunks,
                     scratch_dev, scratch_dev + nub);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(normal_pair_unpack_kernel, dim3((unsigned)((nub + 63) / 64)), dim3(64), 0, (hipStream_t)stream, scratch_dev, scratch_dev + nub, nub,
                     out_dev);
  return (int)hipGetLastError();
}

// plain evaluation: n pairs (ua, ub) -> (z0, z1), one lane per record (in / out: device pointers, 2 floats per record)
namespace {
__global__ __launch_bounds__(64) void normal_pair_kernel(const float* __restrict__ in, float* __restrict__ out, int n) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n) return;
  float z0, z1;
  orr::normal_pair(in[2 * (size_t)i], in[2 * (size_t)i + 1], &z0, &z1);
  out[2 * (size_t)i] = z0; out[2 * (size_t)i + 1] = z1;
}
}  // namespace
extern "C" int orrp_normal_pair(const void* in, void* out, int n, void* stream) {
  if (n <= 0 || !in || !out) return -1;
  hipLaunchKernelGGL(normal_pair_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const float*)in, (float*)out, n);
  return (int)hipGetLastError();
}
