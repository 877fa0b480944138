// orr_learner.hip -- the non-GEMM part of one PPO minibatch update (include/openroborl_learner.h).
//
// Reference: the TF1 graph of agents/ppo_imitation.py:156-258 (loss :196-208) and MpiAdam (stable_baselines/common/mpi_adam.py:40-62).
// The six forward and ten backward contractions of the two 160 -> 512 -> 256 -> {12, 1} networks are library GEMMs issued by the
// host side (openroborl_amd/learner_hip.py); everything between them is here.  All of it is HBM-bound streaming over [m][c] float32
// activations (m = 16384, c = 512: 33.5 MB per tensor), so the rules are: touch every activation once, 16 bytes per lane, no float
// atomics (column sums go through per-block partials that a second small launch adds in a fixed order).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/openroborl_learner.h"

int orr_fail(int code, const char* msg, hipError_t e);  // orr_kernels.hip

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = 32;     // activation rows per workgroup: m = 16384 -> 512 workgroups (two per CU), partials [512][c]
constexpr int kHeadCols = 16;         // head partials per workgroup: 12 actor bias gradients, 1 critic, surrogate sum, value-loss sum, spare
constexpr int kAct = 12;

__device__ inline float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  return x;
}

// ---- what the one-thread-per-sample loss heads and their single-workgroup finish kernels share -----------------------------------------
// The end of a head: a thread's USED sums -> the workgroup's row of partials [block][COLS], the columns from USED on zero.  A wave's sum per
// column, lane 0 of each wave to LDS, one barrier, the four waves combined in a fixed order.
template <int COLS, int USED>
__device__ __forceinline__ void head_partials(const float (&acc)[USED], float* __restrict__ partials) {
  __shared__ float red[kThreads / 64][COLS];
#pragma unroll
  for (int k = 0; k < USED; k++) {
    const float s = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < COLS)
    partials[(size_t)blockIdx.x * COLS + threadIdx.x] =
        threadIdx.x < USED ? (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]) : 0.0f;
}

// The opening of a finish kernel (4 * COLS threads, thread = part * COLS + col): COLS columns x 4 interleaved row groups of the nblk rows,
// combined in a fixed order.  The threads of part 0 get their column's total (the others 0) and route it to its output.
template <int COLS>
__device__ __forceinline__ float head_total(const float* __restrict__ partials, int nblk, int col, int part) {
  __shared__ float red[4][COLS];
  float s = 0.0f;
  for (int b = part; b < nblk; b += 4) s += partials[(size_t)b * COLS + col];
  red[part][col] = s;
  __syncthreads();
  return part == 0 ? (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]) : 0.0f;
}

// ---- loss head: one thread per sample --------------------------------------------------------------------------------------
// d(-min(r A, clip(r) A)) / dr as autograd forms it (ppo.PPO.update): inside the clip range both branches are the same value and
// together pass -A; outside it the clipped branch is constant, so -A passes only while the unclipped branch is the smaller one.
__global__ __launch_bounds__(kThreads) void ppo_head_kernel(const float* __restrict__ mean, const float* __restrict__ value,
                                                            const float* __restrict__ batch, int M, float inv_var, float log_norm, float clip,
                                                            float vf_coef, float inv_m, float* __restrict__ g_mean,
                                                            float* __restrict__ g_value, float* __restrict__ partials) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  float acc[kHeadCols - 1];
#pragma unroll
  for (int k = 0; k < kHeadCols - 1; k++) acc[k] = 0.0f;
  if (i < M) {
    const f4* b4 = reinterpret_cast<const f4*>(batch + (size_t)i * ORR_PPO_BATCH_COLS);
    const f4* m4 = reinterpret_cast<const f4*>(mean + (size_t)i * kAct);
    const f4 a0 = b4[0], a1 = b4[1], a2 = b4[2], rest = b4[3];
    const f4 m0 = m4[0], m1 = m4[1], m2 = m4[2];
    float d[kAct] = {a0.x - m0.x, a0.y - m0.y, a0.z - m0.z, a0.w - m0.w, a1.x - m1.x, a1.y - m1.y, a1.z - m1.z, a1.w - m1.w,
                     a2.x - m2.x, a2.y - m2.y, a2.z - m2.z, a2.w - m2.w};
    float sq = 0.0f;
#pragma unroll
    for (int k = 0; k < kAct; k++) sq += d[k] * d[k];
    const float old_logp = rest.x, A = rest.y, ret = rest.z;
    const float logp = -0.5f * sq * inv_var + log_norm;
    const float ratio = expf(logp - old_logp);
    const float lo = 1.0f - clip, hi = 1.0f + clip;
    const float s1 = ratio * A, s2 = fminf(fmaxf(ratio, lo), hi) * A;
    const bool inside = ratio >= lo && ratio <= hi;
    const float dr = (inside || s1 < s2) ? -A : 0.0f;
    const float gl = dr * ratio * inv_m * inv_var;            // d loss / d logp  x  1 / var
    float gm[kAct];
#pragma unroll
    for (int k = 0; k < kAct; k++) { gm[k] = gl * d[k]; acc[k] = gm[k]; }
    f4* o4 = reinterpret_cast<f4*>(g_mean + (size_t)i * kAct);
    o4[0] = f4{gm[0], gm[1], gm[2], gm[3]}; o4[1] = f4{gm[4], gm[5], gm[6], gm[7]}; o4[2] = f4{gm[8], gm[9], gm[10], gm[11]};
    const float dv = value[i] - ret;
    const float gv = vf_coef * 2.0f * dv * inv_m;
    g_value[i] = gv;
    acc[12] = gv; acc[13] = -fminf(s1, s2); acc[14] = dv * dv;
  }
  head_partials<kHeadCols>(acc, partials);
}

__global__ __launch_bounds__(64) void ppo_head_finish_kernel(const float* __restrict__ partials, int nblk, float inv_m, float* __restrict__ gb_mean,
                                                             float* __restrict__ gb_value, float* __restrict__ stats) {
  const int col = threadIdx.x & 15, part = threadIdx.x >> 4;
  const float t = head_total<kHeadCols>(partials, nblk, col, part);
  if (part == 0) {
    if (col < kAct) gb_mean[col] = t;
    else if (col == 12) gb_value[0] = t;
    else if (col == 13) stats[0] = t * inv_m;
    else if (col == 14) stats[1] = t * inv_m;
  }
}

// ---- loss head with a learned, state-independent log-std (orr_ppo_head_logstd): ppo_head_kernel with a per-dimension std read from the
// device, the entropy bonus and the two diagnostics.  Partials [block][32]: 0..11 the actor's bias gradient, 12 the critic's, 13 surrogate,
// 14 value loss, 15 (r - 1) - log r, 16 clipped samples, 17..28 d surrogate / d log_std, 29..31 zero.
constexpr int kLsCols = 32;
constexpr int kLsUsed = 29;
constexpr double kLog2Pi = 1.8378770664093454836;
// The log-density's constant - sum_k log_std_k - 6 log(2 pi): twelve uniform values of ~-2 each, so a float sum would carry the rounding of a
// ~25 into every sample's ratio; summed in double (twelve adds per thread) it is one rounding of the result.
__device__ inline float log_norm_of(const float* __restrict__ log_std) {
  double s = 6.0 * kLog2Pi;
#pragma unroll
  for (int k = 0; k < kAct; k++) s += (double)log_std[k];
  return (float)-s;
}

__global__ __launch_bounds__(kThreads) void ppo_head_logstd_kernel(const float* __restrict__ mean, const float* __restrict__ value,
                                                                   const float* __restrict__ batch, const float* __restrict__ log_std, int M,
                                                                   float clip, float vf_coef, float inv_m, float* __restrict__ g_mean,
                                                                   float* __restrict__ g_value, float* __restrict__ partials) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  float acc[kLsUsed];
#pragma unroll
  for (int k = 0; k < kLsUsed; k++) acc[k] = 0.0f;
  if (i < M) {
    float inv_std[kAct];
#pragma unroll
    for (int k = 0; k < kAct; k++) inv_std[k] = expf(-log_std[k]);
    const float log_norm = log_norm_of(log_std);
    const f4* b4 = reinterpret_cast<const f4*>(batch + (size_t)i * ORR_PPO_BATCH_COLS);
    const f4* m4 = reinterpret_cast<const f4*>(mean + (size_t)i * kAct);
    const f4 a0 = b4[0], a1 = b4[1], a2 = b4[2], rest = b4[3];
    const f4 m0 = m4[0], m1 = m4[1], m2 = m4[2];
    const float d[kAct] = {a0.x - m0.x, a0.y - m0.y, a0.z - m0.z, a0.w - m0.w, a1.x - m1.x, a1.y - m1.y, a1.z - m1.z, a1.w - m1.w,
                           a2.x - m2.x, a2.y - m2.y, a2.z - m2.z, a2.w - m2.w};
    float z[kAct], sq = 0.0f;
#pragma unroll
    for (int k = 0; k < kAct; k++) { z[k] = d[k] * inv_std[k]; sq += z[k] * z[k]; }
    const float old_logp = rest.x, A = rest.y, ret = rest.z;
    const float logp = -0.5f * sq + log_norm;
    const float log_ratio = logp - old_logp;
    const float ratio = expf(log_ratio);
    const float lo = 1.0f - clip, hi = 1.0f + clip;
    const float s1 = ratio * A, s2 = fminf(fmaxf(ratio, lo), hi) * A;
    const bool inside = ratio >= lo && ratio <= hi;
    const float dr = (inside || s1 < s2) ? -A : 0.0f;
    const float gl = dr * ratio * inv_m;                      // d loss / d logp
    float gm[kAct];
#pragma unroll
    for (int k = 0; k < kAct; k++) {
      gm[k] = gl * z[k] * inv_std[k];
      acc[k] = gm[k];
      acc[17 + k] = gl * (z[k] * z[k] - 1.0f);                // d logp / d log_std_k = z_k^2 - 1
    }
    f4* o4 = reinterpret_cast<f4*>(g_mean + (size_t)i * kAct);
    o4[0] = f4{gm[0], gm[1], gm[2], gm[3]}; o4[1] = f4{gm[4], gm[5], gm[6], gm[7]}; o4[2] = f4{gm[8], gm[9], gm[10], gm[11]};
    const float dv = value[i] - ret;
    const float gv = vf_coef * 2.0f * dv * inv_m;
    g_value[i] = gv;
    acc[12] = gv; acc[13] = -fminf(s1, s2); acc[14] = dv * dv;
    acc[15] = (ratio - 1.0f) - log_ratio; acc[16] = inside ? 0.0f : 1.0f;
  }
  head_partials<kLsCols>(acc, partials);
}

__global__ __launch_bounds__(4 * kLsCols) void ppo_head_logstd_finish_kernel(const float* __restrict__ partials, int nblk, float m, float ent_coef,
                                                                             const float* __restrict__ log_std, float* __restrict__ gb_mean,
                                                                             float* __restrict__ gb_value, float* __restrict__ g_logstd,
                                                                             float* __restrict__ stats) {
  const int col = threadIdx.x & (kLsCols - 1), part = threadIdx.x / kLsCols;
  const float t = head_total<kLsCols>(partials, nblk, col, part);
  if (part == 0) {
    const float inv_m = 1.0f / m;
    if (col < kAct) gb_mean[col] = t;
    else if (col == 12) gb_value[0] = t;
    else if (col == 13) stats[0] = t * inv_m;
    else if (col == 14) stats[1] = t * inv_m;
    else if (col == 15) stats[3] = t * inv_m;
    else if (col == 16) stats[4] = t / m;                     // a count over m: the nearest float to the fraction
    else if (col < 17 + kAct) g_logstd[col - 17] = t - ent_coef;   // - ent_coef dH / d log_std_k, once
    else if (col == 29) {                                     // H = sum_k log_std_k + 6 log(2 pi e)
      stats[2] = 6.0f - log_norm_of(log_std);
    }
  }
}

// ---- the sampler's half of a learned std (orr_gauss_prepare): one thread per row of 12, three 16-byte accesses each way.  A thread reads
// its whole row before it writes it, so scaled may be noise itself (hence no __restrict__ on the two).
__global__ __launch_bounds__(kThreads) void gauss_prepare_kernel(const float* noise, const float* __restrict__ log_std, float* scaled,
                                                                 float* __restrict__ logp, long long n) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float sd[kAct];
#pragma unroll
  for (int k = 0; k < kAct; k++) sd[k] = expf(log_std[k]);
  const f4* x4 = reinterpret_cast<const f4*>(noise + i * kAct);
  const f4 x0 = x4[0], x1 = x4[1], x2 = x4[2];
  f4* o4 = reinterpret_cast<f4*>(scaled + i * kAct);
  o4[0] = f4{sd[0] * x0.x, sd[1] * x0.y, sd[2] * x0.z, sd[3] * x0.w};
  o4[1] = f4{sd[4] * x1.x, sd[5] * x1.y, sd[6] * x1.z, sd[7] * x1.w};
  o4[2] = f4{sd[8] * x2.x, sd[9] * x2.y, sd[10] * x2.z, sd[11] * x2.w};
  if (logp) {
    const float sq = ((x0.x * x0.x + x0.y * x0.y) + (x0.z * x0.z + x0.w * x0.w)) + ((x1.x * x1.x + x1.y * x1.y) + (x1.z * x1.z + x1.w * x1.w)) +
                     ((x2.x * x2.x + x2.y * x2.y) + (x2.z * x2.z + x2.w * x2.w));
    logp[i] = -0.5f * sq + log_norm_of(log_std);
  }
}

// ---- distillation loss head: one thread per sample, the same partials layout (columns 0..11 the bias gradient, 12 the squared error) --------
__global__ __launch_bounds__(kThreads) void distill_head_kernel(const float* __restrict__ mean, const float* __restrict__ target, int M, float inv_m,
                                                                float* __restrict__ g_mean, float* __restrict__ partials) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  float acc[kAct + 1];
#pragma unroll
  for (int k = 0; k < kAct + 1; k++) acc[k] = 0.0f;
  if (i < M) {
    const f4* m4 = reinterpret_cast<const f4*>(mean + (size_t)i * kAct);
    const f4* t4 = reinterpret_cast<const f4*>(target + (size_t)i * kAct);
    const f4 d0 = m4[0] - t4[0], d1 = m4[1] - t4[1], d2 = m4[2] - t4[2];
    const float d[kAct] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w, d2.x, d2.y, d2.z, d2.w};
    float sq = 0.0f;
#pragma unroll
    for (int k = 0; k < kAct; k++) { sq += d[k] * d[k]; acc[k] = 2.0f * d[k] * inv_m; }
    acc[kAct] = sq;
    f4* o4 = reinterpret_cast<f4*>(g_mean + (size_t)i * kAct);
    o4[0] = f4{acc[0], acc[1], acc[2], acc[3]}; o4[1] = f4{acc[4], acc[5], acc[6], acc[7]}; o4[2] = f4{acc[8], acc[9], acc[10], acc[11]};
  }
  head_partials<kHeadCols>(acc, partials);
}

__global__ __launch_bounds__(64) void distill_head_finish_kernel(const float* __restrict__ partials, int nblk, float inv_m, float* __restrict__ gb_mean,
                                                                 float* __restrict__ stats) {
  const int col = threadIdx.x & 15, part = threadIdx.x >> 4;
  const float t = head_total<kHeadCols>(partials, nblk, col, part);
  if (part == 0) {
    if (col < kAct) gb_mean[col] = t;
    else if (col == kAct) stats[0] = t * inv_m;
  }
}

// ---- regression loss head (orr_regress_head): squared error of c <= 64 columns.  16 threads per row (a thread owns four adjacent columns: one
// 16-byte access per tensor and row), 16 rows per pass, kRegRows rows per workgroup; partials [block][c] of the column sums and [block] of the
// loss, added up by colsum_finish_kernel in its fixed order.
constexpr int kRegRows = 64;
constexpr int kRegMaxCols = 64;
__global__ __launch_bounds__(kThreads) void regress_head_kernel(const float* __restrict__ pred, const float* __restrict__ target, int M, int C, float inv_m,
                                                                float* __restrict__ g, float* __restrict__ partials, float* __restrict__ loss_part) {
  __shared__ f4 red[kThreads];
  __shared__ float sq_red[kThreads / 64];
  const int q = threadIdx.x & 15, rsub = threadIdx.x >> 4;
  const int row0 = blockIdx.x * kRegRows;
  const float scale = 2.0f * inv_m;
  f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  float sq = 0.0f;
  if (4 * q < C) {
    for (int r = rsub; r < kRegRows; r += kThreads / 16) {
      const int i = row0 + r;
      if (i >= M) break;
      const size_t o = (size_t)i * C + 4 * q;
      const f4 d = *reinterpret_cast<const f4*>(pred + o) - *reinterpret_cast<const f4*>(target + o);
      const f4 gv = d * scale;
      *reinterpret_cast<f4*>(g + o) = gv;
      acc += gv;
      sq += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
    }
  }
  red[threadIdx.x] = acc;
  const float s = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) sq_red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (rsub == 0 && 4 * q < C) {
    f4 t = red[q];
    for (int k = 1; k < kThreads / 16; k++) t += red[16 * k + q];
    *reinterpret_cast<f4*>(partials + (size_t)blockIdx.x * C + 4 * q) = t;
  }
  if (threadIdx.x == 0) loss_part[blockIdx.x] = ((sq_red[0] + sq_red[1]) + (sq_red[2] + sq_red[3])) * inv_m;
}

// ---- ReLU mask (+ the gradient through an output layer of fan-out K) + per-block column sums ------------------------------
// A workgroup owns kRowsPerBlock rows and all c columns; a thread owns four adjacent columns (one 16-byte access per tensor and
// row) of every (256 / (c/4))-th row.  K = 0: g holds the incoming gradient and is masked in place.  K > 0 (the layer below an
// output layer of fan-out K): the incoming gradient is gy . w^T formed on the fly, and since h and gy are in registers anyway the
// output layer's weight gradient h^T gy is accumulated as well (a library GEMM with N = 12 or 1 and K = the batch runs at 1 % of
// the chip: 100 us for 0.1 GFLOP) - wpart [block][c][K].
template <int K>
__global__ __launch_bounds__(kThreads) void relu_backward_kernel(float* __restrict__ g, const float* __restrict__ h, const float* __restrict__ gy,
                                                                 const float* __restrict__ w, int M, int C, float* __restrict__ partials,
                                                                 float* __restrict__ wpart) {
  constexpr int KK = K > 0 ? K : 1;
  __shared__ f4 red[kThreads];
  __shared__ float wred[K > 0 ? kThreads * 4 * KK : 1];
  const int c4n = C >> 2, side = kThreads / c4n;
  const int c4 = threadIdx.x % c4n, rsub = threadIdx.x / c4n;
  const int row0 = blockIdx.x * kRowsPerBlock;
  float wr[4][KK], gw[4][KK];
  if (K > 0) {
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int k = 0; k < K; k++) { wr[q][k] = w[(size_t)(4 * c4 + q) * K + k]; gw[q][k] = 0.0f; }
  }
  f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
  for (int r = rsub; r < kRowsPerBlock; r += side) {
    const int i = row0 + r;
    if (i >= M) break;
    const size_t o = (size_t)i * C + 4 * c4;
    const f4 hv = *reinterpret_cast<const f4*>(h + o);
    f4 gv;
    if (K > 0) {
      float y[KK];
      if (K % 4 == 0) {
#pragma unroll
        for (int k = 0; k < K / 4; k++) {
          const f4 t = reinterpret_cast<const f4*>(gy + (size_t)i * K)[k];
          y[4 * k] = t.x; y[4 * k + 1] = t.y; y[4 * k + 2] = t.z; y[4 * k + 3] = t.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < K; k++) y[k] = gy[(size_t)i * K + k];
      }
      float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int k = 0; k < K; k++) {
#pragma unroll
        for (int q = 0; q < 4; q++) s[q] = fmaf(y[k], wr[q][k], s[q]);
        gw[0][k] = fmaf(hv.x, y[k], gw[0][k]); gw[1][k] = fmaf(hv.y, y[k], gw[1][k]);
        gw[2][k] = fmaf(hv.z, y[k], gw[2][k]); gw[3][k] = fmaf(hv.w, y[k], gw[3][k]);
      }
      gv = f4{s[0], s[1], s[2], s[3]};
    } else {
      gv = *reinterpret_cast<const f4*>(g + o);
    }
    gv.x = hv.x > 0.0f ? gv.x : 0.0f; gv.y = hv.y > 0.0f ? gv.y : 0.0f;
    gv.z = hv.z > 0.0f ? gv.z : 0.0f; gv.w = hv.w > 0.0f ? gv.w : 0.0f;
    *reinterpret_cast<f4*>(g + o) = gv;
    acc += gv;
  }
  red[threadIdx.x] = acc;
  if (K > 0) {
    // [rsub][q * K + k][c4]: consecutive lanes, consecutive words
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int k = 0; k < K; k++) wred[(rsub * 4 * KK + q * KK + k) * c4n + c4] = gw[q][k];
  }
  __syncthreads();
  if (rsub == 0) {
    f4 t = red[c4];
    for (int s = 1; s < side; s++) t += red[s * c4n + c4];
    *reinterpret_cast<f4*>(partials + (size_t)blockIdx.x * C + 4 * c4) = t;
  }
  if (K > 0) {
    // every thread finishes 4 K / side of this workgroup's c x K sums; wpart[block][(4 c4 + q) * K + k]
    float* o = wpart + (size_t)blockIdx.x * C * K;
    for (int e = rsub; e < 4 * K; e += side) {
      float t = wred[e * c4n + c4];
      for (int s = 1; s < side; s++) t += wred[(s * 4 * KK + e) * c4n + c4];
      o[(size_t)(4 * c4 + e / K) * K + (e % K)] = t;
    }
  }
}

// out[col] = sum over the nblk partial rows of a job: 16 columns per workgroup x 16 interleaved row groups (a thread adds
// nblk / 16 values through four independent accumulators), combined in a fixed order.  Up to 12 jobs per launch; a workgroup finds
// its job in the prefix table of workgroup counts.
constexpr int kMaxJobs = ORR_COLSUM_MAX_JOBS;
constexpr int kFewRows = 16;
struct FinishJobs {
  const float* partials[kMaxJobs];
  float* out[kMaxJobs];
  int nblk[kMaxJobs], cols[kMaxJobs], first[kMaxJobs + 1];
};
__global__ __launch_bounds__(kThreads) void colsum_finish_kernel(FinishJobs J, int n_jobs) {
  __shared__ float red[16][17];
  int job = 0;
  while (job + 1 < n_jobs && (int)blockIdx.x >= J.first[job + 1]) job++;
  const float* __restrict__ partials = J.partials[job];
  const int nblk = J.nblk[job], C = J.cols[job];
  if (nblk <= kFewRows) {      // few rows of many columns (the 16 partial products of a split weight gradient): a thread per column
    const int col = ((int)blockIdx.x - J.first[job]) * kThreads + threadIdx.x;
    if (col >= C) return;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (int b = 0; b < nblk; b++) s[b & 3] += partials[(size_t)b * C + col];
    J.out[job][col] = (s[0] + s[1]) + (s[2] + s[3]);
    return;
  }
  const int lc = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int col = ((int)blockIdx.x - J.first[job]) * 16 + lc;
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (col < C) {
    int b = part;
    for (; b + 48 < nblk; b += 64) {
#pragma unroll
      for (int u = 0; u < 4; u++) s[u] += partials[(size_t)(b + 16 * u) * C + col];
    }
    for (int u = 0; b < nblk; b += 16, u++) s[u & 3] += partials[(size_t)b * C + col];
  }
  red[part][lc] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  if (part == 0 && col < C) {
    float t = 0.0f;
#pragma unroll
    for (int q = 0; q < 16; q++) t += red[q][lc];
    J.out[job][col] = t;
  }
}

// ---- Adam on the flat parameter vector ----------------------------------------------------------------------------------------
// Every workgroup reads the step count when it starts; the LAST one to finish (ticket) advances it, so a captured launch replays.
constexpr int kAdamThreads = 64;     // 434 k parameters = 1700 one-wave workgroups: enough of them in flight to cover the load latency
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                          long long n, float lr, float b1, float b2, float eps, float gscale, int flags,
                                          int* __restrict__ state) {
  const int t = __atomic_load_n(&state[0], __ATOMIC_RELAXED) + 1;
  const float bc1 = 1.0f - powf(b1, (float)t), bc2 = 1.0f - powf(b2, (float)t);
  const float sq2 = sqrtf(bc2);
  const float step = (flags & ORR_ADAM_MPI_EPSILON) ? lr * sq2 / bc1 : lr / bc1;
  const float vs = (flags & ORR_ADAM_MPI_EPSILON) ? 1.0f : 1.0f / sq2;
  const long long i4 = ((long long)blockIdx.x * kAdamThreads + threadIdx.x) * 4;
  if (i4 + 3 < n) {
    f4 gg = *reinterpret_cast<const f4*>(g + i4) * gscale;
    f4 mm = *reinterpret_cast<f4*>(m + i4), vv = *reinterpret_cast<f4*>(v + i4), pp = *reinterpret_cast<f4*>(p + i4);
    mm = mm + (gg - mm) * (1.0f - b1);
    vv = vv * b2 + gg * gg * (1.0f - b2);
    pp.x -= step * mm.x / (sqrtf(vv.x) * vs + eps); pp.y -= step * mm.y / (sqrtf(vv.y) * vs + eps);
    pp.z -= step * mm.z / (sqrtf(vv.z) * vs + eps); pp.w -= step * mm.w / (sqrtf(vv.w) * vs + eps);
    *reinterpret_cast<f4*>(m + i4) = mm; *reinterpret_cast<f4*>(v + i4) = vv; *reinterpret_cast<f4*>(p + i4) = pp;
  } else {
    for (long long i = i4; i < n; i++) {
      const float gg = g[i] * gscale;
      const float mm = m[i] + (gg - m[i]) * (1.0f - b1), vv = v[i] * b2 + gg * gg * (1.0f - b2);
      m[i] = mm; v[i] = vv;
      p[i] -= step * mm / (sqrtf(vv) * vs + eps);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int ticket = atomicAdd(&state[1], 1);
    if (ticket == (int)gridDim.x - 1) {
      __atomic_store_n(&state[0], t, __ATOMIC_RELAXED);
      __atomic_store_n(&state[1], 0, __ATOMIC_RELAXED);
    }
  }
}

__global__ __launch_bounds__(kAdamThreads) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, long long n, float lr, float b1, float b2, float eps, float gscale,
                                                        int flags, int* __restrict__ state) {
  adam_body(p, g, m, v, n, lr, b1, b2, eps, gscale, flags, state);
}

// orr_adam_step_ctl: the same step with its controls read from the device.  Every workgroup reads the record (written earlier on the stream:
// no workgroup of this launch writes it); a set skip word ends them all before the first load, so nobody takes a ticket and state stands.
// Times 1.0f is exact: the neutral record gives adam_kernel's bits.
__global__ __launch_bounds__(kAdamThreads) void adam_ctl_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, long long n, float lr, float b1, float b2, float eps,
                                                            float gscale, int flags, int* __restrict__ state, const orr_update_ctl* __restrict__ ctl) {
  if (ctl->skip != 0) return;
  adam_body(p, g, m, v, n, lr * ctl->lr_mult * ctl->kl_lr_mult, b1, b2, eps, gscale * ctl->grad_scale, flags, state);
}

// ---- the update controls: gradient norm -> clip coefficient, non-finite guard, KL gate (orr_update_control) ---------------------------------
// One streaming pass over the flat gradient (434 k floats = 1.7 MB for PPO): 16-byte loads, two of them in flight per lane, 1024 floats per
// two-wave workgroup = 425 workgroups for PPO (the launch is latency-bound like adam_kernel's: many small workgroups cover it).  A workgroup's
// sum of squares goes to partials[blockIdx.x]; a second one-wave launch adds the partials in index order and writes the record, so the order
// of every addition is fixed by n alone: no float atomics, no ticket, the same inputs give the same bits.
// Error bound of the sum of squares S (all terms >= 0, so every rounding is relative to a partial sum <= S): the longest chain of roundings
// a term passes is 1 (its square) + 2 (the four of a load) + 1 (the lane's two loads) + 6 (wave tree) + 1 (the two waves) = 11 in the first
// launch, ceil(P / 64) (a lane's partials, one after the other) + 6 (wave tree) in the second, P = ceil(n / 1024):
//   |S - S_exact| <= (17 + ceil(P / 64)) * 2^-24 * S_exact        (n = 434701: P = 425, 24 * 2^-24 = 1.4e-6)
// A square above 3.4e38 (|x| > 1.8e19) or a sum that passes it overflows to Inf: the norm then counts as non-finite like a NaN or Inf element.
constexpr int kCtlThreads = 128, kCtlLoads = 2;
constexpr int kCtlBlockFloats = kCtlThreads * 4 * kCtlLoads;
static_assert(kCtlBlockFloats == ORR_UPDATE_CONTROL_BLOCK_FLOATS, "the header's partials count");
static_assert(sizeof(orr_update_ctl) == 48 && alignof(orr_update_ctl) == 16, "orr_update_ctl: twelve 32-bit words, 16-byte aligned");

__device__ inline float sumsq4(f4 a) { return (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w); }

__global__ __launch_bounds__(kCtlThreads) void grad_sumsq_kernel(const float* __restrict__ g, long long n, float* __restrict__ partials) {
  __shared__ float red[kCtlThreads / 64];
  const long long base = (long long)blockIdx.x * kCtlBlockFloats + (long long)threadIdx.x * 4;
  f4 a[kCtlLoads];
#pragma unroll
  for (int u = 0; u < kCtlLoads; u++) {
    const long long i4 = base + (long long)u * kCtlThreads * 4;
    if (i4 + 3 < n) {
      a[u] = *reinterpret_cast<const f4*>(g + i4);
    } else {          // the tail: nothing at or beyond n is read
      a[u] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      if (i4 < n) a[u].x = g[i4];
      if (i4 + 1 < n) a[u].y = g[i4 + 1];
      if (i4 + 2 < n) a[u].z = g[i4 + 2];
    }
  }
  const float s = wave_sum(sumsq4(a[0]) + sumsq4(a[1]));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1];
}

__device__ inline bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(64) void update_control_kernel(const float* __restrict__ partials, long long nparts, float pre_scale, float max_norm,
                                                            const float* __restrict__ kl_ptr, float kl_stop, float kl_target, float kl_lr_lo,
                                                            float kl_lr_hi, orr_update_ctl* __restrict__ ctl) {
  float s = 0.0f;
  for (long long b = threadIdx.x; b < nparts; b += 64) s += partials[b];
  s = wave_sum(s);
  if (threadIdx.x != 0) return;
  const float norm = pre_scale * sqrtf(s);
  const float kl = kl_ptr ? *kl_ptr : 0.0f;
  const bool bad = !finite_f(s) || !finite_f(norm) || !finite_f(kl);
  int skip = (ctl->skip & 2) | (bad ? 1 : 0);
  if (!bad && kl_stop > 0.0f && kl > kl_stop) skip |= 2;
  if (skip == 0 && kl_target > 0.0f) {         // the rsl_rl rule, once per step that is taken
    float mult = ctl->kl_lr_mult;
    if (kl > 2.0f * kl_target) mult = fmaxf(kl_lr_lo, mult / 1.5f);
    else if (kl > 0.0f && kl < 0.5f * kl_target) mult = fminf(kl_lr_hi, mult * 1.5f);
    ctl->kl_lr_mult = mult;
  }
  float scale = 1.0f;
  if (bad) {
    scale = 0.0f;
    ctl->n_nonfinite += 1;
  } else {
    if (max_norm > 0.0f) scale = fminf(1.0f, max_norm / (norm + 1e-6f));
    if (scale < 1.0f) ctl->n_clipped += 1;
    ctl->grad_norm_max = fmaxf(ctl->grad_norm_max, norm);
    ctl->grad_norm_sum += norm;
    ctl->n_calls += 1;
  }
  if (skip & 2) ctl->n_kl_skipped += 1;
  ctl->grad_norm = norm;
  ctl->grad_scale = scale;
  ctl->skip = skip;
}

// ---- running observation normalisation: orr_running_stats_update, orr_normalize_rows ---------------------------------------------------
// The streaming pass.  A workgroup's kStatThreads / (d / 4) * (d / 4) working threads read consecutive 16-byte quads: thread t of pass p
// reads quad t of the pass's rows, so a pass is ONE contiguous range of x (d = 160: 40 column groups x 8 rows = 320 threads = 5120 bytes) and
// a thread keeps its column group over all passes.  A thread's loads of eight passes are issued before the first is used.  The moments are
// shifted sums around the batch's first row s: S1 = sum (x - s), S2 = sum (x - s)^2, float32 over a thread's <= 32 rows, then over the
// workgroup's row groups one after the other.  For a column of offset 1000 and spread 0.01 every x - s is exact and of the spread's size:
// the offset never enters a sum.  Launch-bound partial sums [block][2][d]; 262144 x 160: 1024 workgroups, 1.3 MB of partials behind 168 MB.
constexpr int kStatThreads = ORR_RUNNING_STATS_THREADS, kStatPasses = ORR_RUNNING_STATS_PASSES, kStatUnroll = 8;
static_assert(kStatPasses % kStatUnroll == 0, "whole groups of loads");

__device__ inline void stat_add(f4& s1, f4& s2, f4 v, f4 shift) {
  const f4 e = v - shift;
  s1 += e;
  s2.x = fmaf(e.x, e.x, s2.x); s2.y = fmaf(e.y, e.y, s2.y); s2.z = fmaf(e.z, e.z, s2.z); s2.w = fmaf(e.w, e.w, s2.w);
}

__global__ __launch_bounds__(kStatThreads) void running_stats_partial_kernel(const float* __restrict__ x, long long n, int d,
                                                                            float* __restrict__ partials) {
  __shared__ f4 red1[kStatThreads];
  __shared__ f4 red2[kStatThreads];
  const int c4n = d >> 2, side = kStatThreads / c4n, t = threadIdx.x;
  const int c4 = t % c4n, r = t / c4n;
  f4 s1 = {0.0f, 0.0f, 0.0f, 0.0f}, s2 = {0.0f, 0.0f, 0.0f, 0.0f};
  const long long first = (long long)blockIdx.x * side * kStatPasses + r;      // this thread's rows: first, first + side, ...
  if (r < side && first < n) {
    const f4 shift = *reinterpret_cast<const f4*>(x + 4 * c4);
    const long long left = (n - first + side - 1) / side;
    const int np = left < kStatPasses ? (int)left : kStatPasses;
    const f4* q = reinterpret_cast<const f4*>(x + first * d + 4 * c4);
    const long long step = (long long)side * c4n;                               // quads from a row to the thread's next
    int p = 0;
    for (; p + kStatUnroll <= np; p += kStatUnroll) {
      f4 v[kStatUnroll];
#pragma unroll
      for (int u = 0; u < kStatUnroll; u++) v[u] = q[(p + u) * step];
#pragma unroll
      for (int u = 0; u < kStatUnroll; u++) stat_add(s1, s2, v[u], shift);
    }
    for (; p < np; p++) stat_add(s1, s2, q[p * step], shift);
  }
  red1[t] = s1;
  red2[t] = s2;
  __syncthreads();
  if (t < c4n) {
    f4 a1 = red1[t], a2 = red2[t];
    for (int k = 1; k < side; k++) { a1 += red1[k * c4n + t]; a2 += red2[k * c4n + t]; }
    float* o = partials + (size_t)blockIdx.x * 2 * d + 4 * t;
    *reinterpret_cast<f4*>(o) = a1;
    *reinterpret_cast<f4*>(o + d) = a2;
  }
}

// The merge: one workgroup.  kMergeThreads / d threads share a column: each adds a consecutive range of the partials in index order, in
// float64, and the ranges are added in their order; then one thread per column does the batch's moments and the merge with the record in
// float64.  Every thread reads the record's count before the barrier, thread 0 writes it behind it.
constexpr int kMergeThreads = 1024;
__global__ __launch_bounds__(kMergeThreads) void running_stats_merge_kernel(const float* __restrict__ partials, long long nparts, long long n, int d,
                                                                           float eps, const float* __restrict__ x, float* __restrict__ rec) {
  __shared__ double red1[kMergeThreads];
  __shared__ double red2[kMergeThreads];
  const int segs = kMergeThreads / d, t = threadIdx.x;
  const int c = t % d, seg = t / d;
  const long long per = (nparts + segs - 1) / segs;
  double a1 = 0.0, a2 = 0.0;
  if (seg < segs) {
    const long long b0 = seg * per, b1 = b0 + per < nparts ? b0 + per : nparts;
#pragma unroll 8
    for (long long b = b0; b < b1; b++) {
      a1 += (double)partials[(size_t)b * 2 * d + c];
      a2 += (double)partials[(size_t)b * 2 * d + d + c];
    }
  }
  red1[t] = a1;
  red2[t] = a2;
  long long* count = reinterpret_cast<long long*>(rec);
  const long long na = *count;
  __syncthreads();
  if (t < d) {
    double S1 = red1[t], S2 = red2[t];
    for (int k = 1; k < segs; k++) { S1 += red1[k * d + t]; S2 += red2[k * d + t]; }
    const double nb = (double)n;
    double mean = (double)x[t] + S1 / nb;
    double M2 = S2 - S1 * S1 / nb;
    M2 = M2 > 0.0 ? M2 : 0.0;
    double tot = nb;
    float* mean_r = rec + ORR_RUNNING_STATS_MEAN(d);
    float* var_r = rec + ORR_RUNNING_STATS_VAR(d);
    float* rstd_r = rec + ORR_RUNNING_STATS_RSTD(d);
    if (na > 0) {
      const double a = (double)na, mean_a = (double)mean_r[t], delta = mean - mean_a;
      tot = a + nb;
      M2 = (double)var_r[t] * a + M2 + delta * delta * (a * nb / tot);
      mean = mean_a + delta * (nb / tot);
    }
    const float var = (float)(M2 / tot);
    mean_r[t] = (float)mean;
    var_r[t] = var;
    rstd_r[t] = (float)(1.0 / (sqrt((double)var) + (double)eps));
  }
  if (t == 0) *count = (na > 0 ? na : 0) + n;
}

// (x - mean) * rstd: a thread owns kNormLoads quads a workgroup's width apart, reads them all, then writes them - out may be x itself
// (no __restrict__ on the two).  A subtraction and a multiplication: nothing for the compiler to contract.
constexpr int kNormLoads = 4;
__global__ __launch_bounds__(kThreads) void normalize_rows_kernel(const float* x, long long quads, int c4n, const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, float* out) {
  const long long base = (long long)blockIdx.x * (kThreads * kNormLoads) + threadIdx.x;
  f4 v[kNormLoads];
#pragma unroll
  for (int u = 0; u < kNormLoads; u++) {
    const long long i = base + (long long)u * kThreads;
    if (i < quads) v[u] = reinterpret_cast<const f4*>(x)[i];
  }
#pragma unroll
  for (int u = 0; u < kNormLoads; u++) {
    const long long i = base + (long long)u * kThreads;
    if (i < quads) {
      const int c4 = (int)(i % c4n);
      const f4 m = reinterpret_cast<const f4*>(mean)[c4], r = reinterpret_cast<const f4*>(rstd)[c4];
      reinterpret_cast<f4*>(out)[i] = (v[u] - m) * r;
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool stats_dims_ok(int d) { return d >= 4 && d <= 256 && (d % 4) == 0; }
inline int nblocks_rows(int m) { return (m + kRowsPerBlock - 1) / kRowsPerBlock; }
inline bool cols_ok(int c) { return c >= 4 && (c % 4) == 0 && (c / 4) <= kThreads && (kThreads % (c / 4)) == 0; }

// behind an entry point's launches: 0, or the entry's failure with the runtime's error behind `who`
int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? orr_fail(-2, who, e) : 0;
}

// the checks and the launch of orr_adam_step (ctl NULL: adam_kernel) and of orr_adam_step_ctl (which has looked at its ctl: adam_ctl_kernel)
int adam_step(const char* who, float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
              float grad_scale, int32_t flags, int32_t* state, const orr_update_ctl* ctl, void* stream) {
  char msg[64];
  const auto fail = [&](const char* what) { snprintf(msg, sizeof(msg), "%s: %s", who, what); return orr_fail(-1, msg, hipSuccess); };
  if (!p || !g || !m || !v || !state || n <= 0) return fail("bad argument");
  if (flags & ~ORR_ADAM_MPI_EPSILON) return fail("unknown flag");
  if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || !aligned16(ctl)) return fail("buffers must be 16-byte aligned");
  const long long per_block = 4LL * kAdamThreads;
  const dim3 grid((unsigned)((n + per_block - 1) / per_block));
  if (ctl)
    hipLaunchKernelGGL(adam_ctl_kernel, grid, dim3(kAdamThreads), 0, (hipStream_t)stream, p, g, m, v, (long long)n, lr, beta1, beta2, eps, grad_scale,
                       (int)flags, (int*)state, ctl);
  else
    hipLaunchKernelGGL(adam_kernel, grid, dim3(kAdamThreads), 0, (hipStream_t)stream, p, g, m, v, (long long)n, lr, beta1, beta2, eps, grad_scale,
                       (int)flags, (int*)state);
  snprintf(msg, sizeof(msg), "%s: launch", who);
  return launched(msg);
}

int launch_finish(FinishJobs& J, int n_jobs, hipStream_t st, const char* who) {
  J.first[0] = 0;
  for (int j = 0; j < n_jobs; j++) J.first[j + 1] = J.first[j] + (J.nblk[j] <= kFewRows ? (J.cols[j] + kThreads - 1) / kThreads : (J.cols[j] + 15) / 16);
  hipLaunchKernelGGL(colsum_finish_kernel, dim3((unsigned)J.first[n_jobs]), dim3(kThreads), 0, st, J, n_jobs);
  return launched(who);
}

}  // namespace

extern "C" {

int32_t orr_learner_partial_rows(int32_t m) { return m > 0 ? nblocks_rows(m) : -1; }

int64_t orr_learner_workspace_floats(int32_t m, int32_t c) {
  if (m <= 0 || c <= 0) return -1;
  const int64_t rows = nblocks_rows(m), head = (m + kThreads - 1) / kThreads;
  const int64_t a = rows * (int64_t)c * (1 + kAct), b = head * kHeadCols;     // orr_head_backward: [rows][c] + [rows][c][12]
  return a > b ? a : b;
}

int32_t orr_ppo_head(const float* mean, const float* value, const float* batch, int32_t m, float std, float clip, float vf_coef,
                     float* g_mean, float* g_value, float* gb_mean, float* gb_value, float* stats, float* workspace, void* stream) {
  if (!mean || !value || !batch || !g_mean || !g_value || !gb_mean || !gb_value || !stats || !workspace || m <= 0 || !(std > 0.0f))
    return orr_fail(-1, "orr_ppo_head: bad argument", hipSuccess);
  if (!aligned16(mean) || !aligned16(batch) || !aligned16(g_mean)) return orr_fail(-1, "orr_ppo_head: buffers must be 16-byte aligned", hipSuccess);
  const float var = std * std;
  const float log_norm = -0.5f * (float)kAct * logf(2.0f * 3.14159265358979323846f * var);
  const int nblk = (m + kThreads - 1) / kThreads;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ppo_head_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, st, mean, value, batch, (int)m, 1.0f / var, log_norm, clip, vf_coef,
                     1.0f / (float)m, g_mean, g_value, workspace);
  hipLaunchKernelGGL(ppo_head_finish_kernel, dim3(1), dim3(64), 0, st, (const float*)workspace, nblk, 1.0f / (float)m, gb_mean, gb_value, stats);
  return launched("orr_ppo_head: launch");
}

int32_t orr_ppo_head_logstd(const float* mean, const float* value, const float* batch, const float* log_std, int32_t m, float clip, float vf_coef,
                            float ent_coef, float* g_mean, float* g_value, float* g_logstd, float* gb_mean, float* gb_value, float* stats,
                            float* workspace, void* stream) {
  if (!mean || !value || !batch || !log_std || !g_mean || !g_value || !g_logstd || !gb_mean || !gb_value || !stats || !workspace || m <= 0 ||
      !(clip >= 0.0f) || !(ent_coef == ent_coef))
    return orr_fail(-1, "orr_ppo_head_logstd: bad argument", hipSuccess);
  if (!aligned16(mean) || !aligned16(batch) || !aligned16(g_mean))
    return orr_fail(-1, "orr_ppo_head_logstd: buffers must be 16-byte aligned", hipSuccess);
  const int nblk = (m + kThreads - 1) / kThreads;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ppo_head_logstd_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, st, mean, value, batch, log_std, (int)m, clip, vf_coef,
                     1.0f / (float)m, g_mean, g_value, workspace);
  hipLaunchKernelGGL(ppo_head_logstd_finish_kernel, dim3(1), dim3(4 * kLsCols), 0, st, (const float*)workspace, nblk, (float)m, ent_coef, log_std,
                     gb_mean, gb_value, g_logstd, stats);
  return launched("orr_ppo_head_logstd: launch");
}

int32_t orr_gauss_prepare(const float* noise, const float* log_std, float* scaled, float* logp, int32_t n, void* stream) {
  if (!noise || !log_std || !scaled || n <= 0) return orr_fail(-1, "orr_gauss_prepare: bad argument", hipSuccess);
  if (!aligned16(noise) || !aligned16(scaled)) return orr_fail(-1, "orr_gauss_prepare: buffers must be 16-byte aligned", hipSuccess);
  const size_t bytes = (size_t)n * kAct * sizeof(float);
  const uintptr_t a = reinterpret_cast<uintptr_t>(noise), b = reinterpret_cast<uintptr_t>(scaled);
  if (a != b && a < b + bytes && b < a + bytes)
    return orr_fail(-1, "orr_gauss_prepare: scaled must be noise itself or not overlap it", hipSuccess);
  hipLaunchKernelGGL(gauss_prepare_kernel, dim3((unsigned)(((long long)n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, noise,
                     log_std, scaled, logp, (long long)n);
  return launched("orr_gauss_prepare: launch");
}

int32_t orr_distill_head(const float* mean, const float* target, int32_t m, float* g_mean, float* gb_mean, float* stats, float* workspace,
                         void* stream) {
  if (!mean || !target || !g_mean || !gb_mean || !stats || !workspace || m <= 0) return orr_fail(-1, "orr_distill_head: bad argument", hipSuccess);
  if (!aligned16(mean) || !aligned16(target) || !aligned16(g_mean)) return orr_fail(-1, "orr_distill_head: buffers must be 16-byte aligned", hipSuccess);
  const int nblk = (m + kThreads - 1) / kThreads;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(distill_head_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, st, mean, target, (int)m, 1.0f / (float)m, g_mean, workspace);
  hipLaunchKernelGGL(distill_head_finish_kernel, dim3(1), dim3(64), 0, st, (const float*)workspace, nblk, 1.0f / (float)m, gb_mean, stats);
  return launched("orr_distill_head: launch");
}

int32_t orr_regress_head(const float* pred, const float* target, int32_t m, int32_t c, float* g, float* gb, float* stats, float* workspace,
                         void* stream) {
  if (!pred || !target || !g || !gb || !stats || !workspace || m <= 0) return orr_fail(-1, "orr_regress_head: bad argument", hipSuccess);
  if (c < 4 || (c % 4) != 0 || c > kRegMaxCols) return orr_fail(-1, "orr_regress_head: c must be a multiple of 4, at most 64", hipSuccess);
  if (!aligned16(pred) || !aligned16(target) || !aligned16(g) || !aligned16(workspace))
    return orr_fail(-1, "orr_regress_head: buffers must be 16-byte aligned", hipSuccess);
  const int nblk = (m + kRegRows - 1) / kRegRows;
  hipStream_t st = (hipStream_t)stream;
  float* loss_part = workspace + (size_t)nblk * c;                // [nblk][c] column sums, then [nblk] shares of the loss
  hipLaunchKernelGGL(regress_head_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, st, pred, target, (int)m, (int)c, 1.0f / (float)m, g, workspace, loss_part);
  if (const int rc = launched("orr_regress_head: launch")) return rc;
  FinishJobs J{};
  J.partials[0] = workspace; J.out[0] = gb; J.nblk[0] = nblk; J.cols[0] = c;
  J.partials[1] = loss_part; J.out[1] = stats; J.nblk[1] = nblk; J.cols[1] = 1;
  return launch_finish(J, 2, st, "orr_regress_head: launch");
}

int32_t orr_relu_backward(float* g, const float* h, int32_t m, int32_t c, float* gb, float* workspace, void* stream) {
  if (!g || !h || !workspace || m <= 0) return orr_fail(-1, "orr_relu_backward: bad argument", hipSuccess);
  if (!cols_ok(c)) return orr_fail(-1, "orr_relu_backward: c must be a multiple of 4 that divides 1024", hipSuccess);
  if (!aligned16(g) || !aligned16(h) || !aligned16(workspace)) return orr_fail(-1, "orr_relu_backward: buffers must be 16-byte aligned", hipSuccess);
  const int nblk = nblocks_rows(m);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(relu_backward_kernel<0>, dim3((unsigned)nblk), dim3(kThreads), 0, st, g, h, (const float*)nullptr, (const float*)nullptr, (int)m,
                     (int)c, workspace, (float*)nullptr);
  if (const int rc = launched("orr_relu_backward: launch")) return rc;
  if (!gb) return 0;                                 // deferred: the caller sums workspace [rows][c] with orr_colsum_finish
  FinishJobs J{};
  J.partials[0] = workspace; J.out[0] = gb; J.nblk[0] = nblk; J.cols[0] = c;
  return launch_finish(J, 1, st, "orr_relu_backward: launch");
}

int32_t orr_head_backward(const float* gy, int32_t k, const float* w, const float* h, int32_t m, int32_t c, float* gz, float* gb, float* gw,
                          float* workspace, void* stream) {
  if (!gy || !w || !h || !gz || !workspace || m <= 0) return orr_fail(-1, "orr_head_backward: bad argument", hipSuccess);
  if (k != 12 && k != 1) return orr_fail(-1, "orr_head_backward: fan-out must be 12 or 1", hipSuccess);
  if (!cols_ok(c)) return orr_fail(-1, "orr_head_backward: c must be a multiple of 4 that divides 1024", hipSuccess);
  if ((gb == nullptr) != (gw == nullptr)) return orr_fail(-1, "orr_head_backward: gb and gw must both be given or both be deferred", hipSuccess);
  if (!aligned16(gy) || !aligned16(h) || !aligned16(gz) || !aligned16(workspace))
    return orr_fail(-1, "orr_head_backward: buffers must be 16-byte aligned", hipSuccess);
  const int nblk = nblocks_rows(m);
  hipStream_t st = (hipStream_t)stream;
  float* wpart = workspace + (size_t)nblk * c;
  if (k == 12)
    hipLaunchKernelGGL(relu_backward_kernel<12>, dim3((unsigned)nblk), dim3(kThreads), 0, st, gz, h, gy, w, (int)m, (int)c, workspace, wpart);
  else
    hipLaunchKernelGGL(relu_backward_kernel<1>, dim3((unsigned)nblk), dim3(kThreads), 0, st, gz, h, gy, w, (int)m, (int)c, workspace, wpart);
  if (const int rc = launched("orr_head_backward: launch")) return rc;
  if (!gb) return 0;                                 // deferred: workspace [rows][c] then [rows][c * k]
  FinishJobs J{};
  J.partials[0] = workspace; J.out[0] = gb; J.nblk[0] = nblk; J.cols[0] = c;
  J.partials[1] = wpart; J.out[1] = gw; J.nblk[1] = nblk; J.cols[1] = c * k;
  return launch_finish(J, 2, st, "orr_head_backward: launch");
}

int32_t orr_colsum_finish(const orr_colsum_job* jobs, int32_t n_jobs, void* stream) {
  if (!jobs || n_jobs < 1 || n_jobs > ORR_COLSUM_MAX_JOBS) return orr_fail(-1, "orr_colsum_finish: 1 to 12 jobs", hipSuccess);
  FinishJobs J{};
  for (int j = 0; j < n_jobs; j++) {
    if (!jobs[j].partials || !jobs[j].out || jobs[j].rows < 1 || jobs[j].cols < 1) return orr_fail(-1, "orr_colsum_finish: bad job", hipSuccess);
    J.partials[j] = jobs[j].partials; J.out[j] = jobs[j].out; J.nblk[j] = jobs[j].rows; J.cols[j] = jobs[j].cols;
  }
  return launch_finish(J, n_jobs, (hipStream_t)stream, "orr_colsum_finish: launch");
}

int32_t orr_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                      float grad_scale, int32_t flags, int32_t* state, void* stream) {
  return adam_step("orr_adam_step", p, g, m, v, n, lr, beta1, beta2, eps, grad_scale, flags, state, nullptr, stream);
}

int32_t orr_sizeof_update_ctl(void) { return (int32_t)sizeof(orr_update_ctl); }

int64_t orr_update_control_partials(int64_t n) { return n > 0 ? (n + kCtlBlockFloats - 1) / kCtlBlockFloats : -1; }

int32_t orr_update_control(const float* g, int64_t n, float pre_scale, float max_norm, const float* kl, float kl_stop, float kl_target,
                           float kl_lr_lo, float kl_lr_hi, float* partials, orr_update_ctl* ctl, void* stream) {
  if (!g || !partials || !ctl || n <= 0) return orr_fail(-1, "orr_update_control: bad argument", hipSuccess);
  if (!aligned16(g) || !aligned16(ctl)) return orr_fail(-1, "orr_update_control: g and ctl must be 16-byte aligned", hipSuccess);
  if ((reinterpret_cast<uintptr_t>(partials) & 3) || (reinterpret_cast<uintptr_t>(kl) & 3))
    return orr_fail(-1, "orr_update_control: partials and kl must be 4-byte aligned", hipSuccess);
  if (!(kl_lr_lo <= kl_lr_hi)) return orr_fail(-1, "orr_update_control: kl_lr_lo must not exceed kl_lr_hi", hipSuccess);
  if (!kl && (kl_stop > 0.0f || kl_target > 0.0f)) return orr_fail(-1, "orr_update_control: a KL threshold needs kl", hipSuccess);
  const long long nparts = (n + kCtlBlockFloats - 1) / kCtlBlockFloats;
  if (nparts > 0x7fffffffLL) return orr_fail(-1, "orr_update_control: n too large", hipSuccess);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nparts), dim3(kCtlThreads), 0, (hipStream_t)stream, g, (long long)n, partials);
  hipLaunchKernelGGL(update_control_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)partials, nparts, pre_scale, max_norm, kl, kl_stop,
                     kl_target, kl_lr_lo, kl_lr_hi, ctl);
  return launched("orr_update_control: launch");
}

int64_t orr_sizeof_running_stats(int32_t d) { return stats_dims_ok(d) ? (int64_t)sizeof(float) * ORR_RUNNING_STATS_FLOATS(d) : -1; }

int64_t orr_running_stats_partials(int64_t n, int32_t d) {
  if (n < 1 || !stats_dims_ok(d)) return -1;
  const int64_t rows = ORR_RUNNING_STATS_BLOCK_ROWS(d);
  return (n + rows - 1) / rows * 2 * d;
}

int32_t orr_running_stats_update(const float* x, int64_t n, int32_t d, float eps, float* rec, float* partials, void* stream) {
  if (!x || !rec || !partials || n < 1) return orr_fail(-1, "orr_running_stats_update: bad argument", hipSuccess);
  if (!stats_dims_ok(d)) return orr_fail(-1, "orr_running_stats_update: d must be a multiple of 4 from 4 to 256", hipSuccess);
  if (!(eps > 0.0f && eps <= 3.4e38f)) return orr_fail(-1, "orr_running_stats_update: eps must be positive and finite", hipSuccess);
  if (!aligned16(x) || !aligned16(rec) || !aligned16(partials))
    return orr_fail(-1, "orr_running_stats_update: x, rec and partials must be 16-byte aligned", hipSuccess);
  const int64_t rows = ORR_RUNNING_STATS_BLOCK_ROWS(d);
  const long long nparts = (n + rows - 1) / rows;
  if (nparts > 0x7fffffffLL) return orr_fail(-1, "orr_running_stats_update: n too large", hipSuccess);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(running_stats_partial_kernel, dim3((unsigned)nparts), dim3(kStatThreads), 0, st, x, (long long)n, (int)d, partials);
  hipLaunchKernelGGL(running_stats_merge_kernel, dim3(1), dim3(kMergeThreads), 0, st, (const float*)partials, nparts, (long long)n, (int)d, eps, x, rec);
  return launched("orr_running_stats_update: launch");
}

int32_t orr_normalize_rows(const float* x, int64_t n, int32_t d, const float* mean, const float* rstd, float* out, void* stream) {
  if (!x || !mean || !rstd || !out || n < 1) return orr_fail(-1, "orr_normalize_rows: bad argument", hipSuccess);
  if (!stats_dims_ok(d)) return orr_fail(-1, "orr_normalize_rows: d must be a multiple of 4 from 4 to 256", hipSuccess);
  if (!aligned16(x) || !aligned16(out) || !aligned16(mean) || !aligned16(rstd))
    return orr_fail(-1, "orr_normalize_rows: buffers must be 16-byte aligned", hipSuccess);
  const long long quads = (long long)n * (d / 4);
  const uintptr_t a = reinterpret_cast<uintptr_t>(x), b = reinterpret_cast<uintptr_t>(out), bytes = (uintptr_t)quads * 16;
  if (a != b && a < b + bytes && b < a + bytes) return orr_fail(-1, "orr_normalize_rows: out must be x itself or not overlap it", hipSuccess);
  const long long per_block = (long long)kThreads * kNormLoads, nblk = (quads + per_block - 1) / per_block;
  if (nblk > 0x7fffffffLL) return orr_fail(-1, "orr_normalize_rows: n too large", hipSuccess);
  hipLaunchKernelGGL(normalize_rows_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, (hipStream_t)stream, x, quads, (int)(d / 4), mean, rstd, out);
  return launched("orr_normalize_rows: launch");
}

int32_t orr_adam_step_ctl(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                          float grad_scale, int32_t flags, int32_t* state, const orr_update_ctl* ctl, void* stream) {
  if (!ctl) return orr_fail(-1, "orr_adam_step_ctl: bad argument", hipSuccess);
  return adam_step("orr_adam_step_ctl", p, g, m, v, n, lr, beta1, beta2, eps, grad_scale, flags, state, ctl, stream);       // its alignment: there
}

}  // extern "C"
