// orr_policy.hip -- fused actor / critic forward pass for all robots of a shard (include/openroborl_policy.h).
//
// Reference: one `policy.step(ob)` per robot with batch 1 (agents/imitation_runners.py:88-92) on the MlpPolicy-style nets
// of agents/imitation_policies.py:44-51,96-107 (run.py:101-105: layers [512, 256], ReLU).  Here one launch does
//   h0 = relu(obs W0 + b0);  h1 = relu(h0 W1 + b1);  out = h1 W2 + b2        for the actor and the critic,
//   action = clip(mean + std * noise)
// on the matrix cores with f32 inputs and f32 accumulation (v_mfma_f32_16x16x4_f32 = a k-ordered fmaf chain).
//
// Mapping: a workgroup (4 wavefronts, one per SIMD) owns 16 robots (rows).  N = 4096 robots -> 256 workgroups = one per CU.
// The 16 x 160 observation tile and the hidden activations (16 x 1024, 16 x 512) live in LDS; the weights are streamed
// from L2 in a fragment-major packing (orr_policy_pack) so that one 16-byte load per lane is the B operand of four
// consecutive k-steps; each wave owns a quarter of every layer's output columns and keeps its accumulators in registers.
// MFMA count per wave: 640 (layer 0) + 1024 (layer 1) + 64 (heads) of 32 cycles each = 23 us at 2.4 GHz; the weight
// stream is 1.7 MB per workgroup out of L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/openroborl_policy.h"
#include "../../include/openroborl_learner.h"   // orr_history_student_head: a learner's launch that needs this file's layer<>

int orr_fail(int code, const char* msg, hipError_t e);  // orr_kernels.hip

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kObs = ORR_POLICY_OBS_DIM, kH0 = ORR_POLICY_H0, kH1 = ORR_POLICY_H1, kAct = ORR_POLICY_ACT_DIM;
constexpr int kRows = 16;                       // robots per workgroup
constexpr int kPriv = ORR_POLICY_PRIV_DIM;      // privileged columns of the critic's input (orr_policy_forward_priv)
constexpr int kH0Stride = 2 * kH0 + 1;          // actor | critic hidden 0 (odd, like the observation tile's stride: forward_kernel)
constexpr int kH1Stride = 2 * kH1 + 1;          // actor | critic hidden 1
constexpr int kHist = ORR_HISTORY_DIM;          // the history encoder (orr_policy_forward_history): 512 -> 256 -> 48
constexpr int kEncH = 256;
constexpr int kHistStride = kHist + 1;          // the 16 x 512 history tile lives where hidden 0 will, the encoder's hidden layer where hidden 1 will
static_assert(kHistStride <= kH0Stride && kEncH + 1 <= kH1Stride && kHist % 64 == 0 && kEncH % 64 == 0, "the encoder's tiles fit the hidden layers' LDS");

__global__ void pack_kernel(const float* __restrict__ w, int K, int N, float* __restrict__ out, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i & 3), l = (int)((i >> 2) & 63);
  const long long t = i >> 8;                   // nt * (K / 16) + kg
  const int kgs = K / 16, kg = (int)(t % kgs), nt = (int)(t / kgs);
  const int k = 16 * kg + 4 * j + (l >> 4), c = 16 * nt + (l & 15);
  out[i] = c < N ? w[(size_t)k * N + c] : 0.0f;
}

// orr_policy_pack_norm: pack_kernel on diag(rstd) W, and behind its workgroups those of the folded bias - a thread per output column walks
// the k rows in order (eight loads in flight, one fmaf chain from +0: with mean 0 every term is a zero and b comes out as it went in).
__global__ __launch_bounds__(256) void pack_norm_kernel(const float* __restrict__ w, int K, int N, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, const float* b, float* __restrict__ out, float* out_b,
                                                        long long total, int pack_blocks) {
  if ((int)blockIdx.x < pack_blocks) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i & 3), l = (int)((i >> 2) & 63);
    const long long t = i >> 8;                 // nt * (K / 16) + kg
    const int kgs = K / 16, kg = (int)(t % kgs), nt = (int)(t / kgs);
    const int k = 16 * kg + 4 * j + (l >> 4), c = 16 * nt + (l & 15);
    out[i] = c < N ? w[(size_t)k * N + c] * rstd[k] : 0.0f;
    return;
  }
  const int c = ((int)blockIdx.x - pack_blocks) * 256 + threadIdx.x;
  if (c >= N) return;
  float s = 0.0f;
  for (int k0 = 0; k0 < K; k0 += 8) {           // K is a multiple of 16
    float wv[8];
#pragma unroll
    for (int u = 0; u < 8; u++) wv[u] = w[(size_t)(k0 + u) * N + c];
#pragma unroll
    for (int u = 0; u < 8; u++) s = fmaf(mean[k0 + u] * rstd[k0 + u], wv[u], s);
  }
  out_b[c] = b[c] - s;
}

struct Params {
  orr_policy_net net;
  const float* obs;
  const float* noise;
  float* action;
  float* raw;
  float* value;
  float* mean;
  int n;
  float std, clip;
  const float* priv;   // forward_kernel<kObs + kPriv, ..> only; LAST: the fields above keep their offsets in the plain kernel's arguments
};
// The history kernel's own arguments (forward_kernel<.., .., true>): Params stays what the three older kernels were compiled against.
struct HistParams : Params {
  orr_history_encoder enc;
  const float* hist;
  float* latent;
};

// acc[t] += A(16 x 16 k-group kg, from LDS) * B(tile t, k-group kg): four k-steps of v_mfma_f32_16x16x4_f32 per tile.
// A fragment of k-step j: lane l holds A[l & 15][16 kg + 4 j + (l >> 4)];  B fragment: element j of the packed float4.
template <int TILES>
__device__ __forceinline__ void mma_group(f32x4 (&acc)[TILES], const float (&a)[4], const f32x4 (&b)[TILES]) {
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int t = 0; t < TILES; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[t][j], acc[t], 0, 0, 0);
}

// One layer for this wave: TILES column tiles starting at tile index `nt0` of a packed K x (16 * ntiles) matrix.
// `act` points at column 0 of the A operand in LDS (row stride `stride`).  The weight stream is software-pipelined
// DEPTH k-groups deep (a k-group = 4 MFMA k-steps = one 16-byte load per lane and tile); the A fragments of the next
// k-group are read from LDS before the MFMAs of the current one.  K / 16 must be a multiple of DEPTH.
// KGS, G0: the call covers k-groups [G0, G0 + K / 16) of a packed matrix of KGS k-groups, `act` pointing at column 16 G0 of the A operand
// (default: all of it) - a matrix whose k-groups are no multiple of the depth is done as two calls.
// UNIT: names the calling kernel's family (forward_kernel passes its KP, the history kernel KP + 1) and is used by nothing: kernels of different families then share
// no instantiation of this function.  Before it is inlined the optimiser folds arguments that all call sites of an instantiation agree
// on (the LDS tile's address among them) into the function; a third kernel calling the privileged kernel's instantiations took that away
// from it and changed its instructions (profiles/teacher_policy.txt).
template <int UNIT, int TILES, int K, int DEPTH, int KGS = K / 16, int G0 = 0>
__device__ __forceinline__ void layer(f32x4 (&acc)[TILES], const float* __restrict__ wp, int nt0, const float* act, int stride, int lane) {
  constexpr int KG = K / 16;
  static_assert(KG % DEPTH == 0, "k-groups must be a multiple of the pipeline depth");
  static_assert(G0 + KG <= KGS, "k-groups of the packed matrix");
  const f32x4* w4 = reinterpret_cast<const f32x4*>(wp) + ((size_t)nt0 * KGS + G0) * 64 + lane;   // tile t, k-group G0 + g: w4[(t * KGS + g) * 64]
  const float* arow = act + (lane & 15) * stride + (lane >> 4);                             // k-group g, k-step j: arow[16 g + 4 j]
  f32x4 b[DEPTH][TILES];
  float a[2][4];
#pragma unroll
  for (int d = 0; d < DEPTH - 1; d++)
#pragma unroll
    for (int t = 0; t < TILES; t++) b[d][t] = w4[(t * KGS + d) * 64];
#pragma unroll
  for (int j = 0; j < 4; j++) a[0][j] = arow[4 * j];
#pragma unroll 1
  for (int g0 = 0; g0 < KG; g0 += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
      const int g = g0 + d;
      if (g + DEPTH - 1 < KG) {
#pragma unroll
        for (int t = 0; t < TILES; t++) b[(d + DEPTH - 1) % DEPTH][t] = w4[(t * KGS + g + DEPTH - 1) * 64];
      }
      if constexpr (DEPTH % 2 == 0) {
        if (g + 1 < KG) {
#pragma unroll
          for (int j = 0; j < 4; j++) a[(d + 1) & 1][j] = arow[16 * (g + 1) + 4 * j];
        }
      } else if (g > 0) {   // an odd depth: d does not tell the parity of g, so no second A buffer - the k-group's own fragments, read here
#pragma unroll
        for (int j = 0; j < 4; j++) a[d & 1][j] = arow[16 * g + 4 * j];
      }
      mma_group<TILES>(acc, a[d & 1], b[d]);
    }
  }
}

// C/D layout of the 16x16 tile: column = lane & 15, row = 4 * (lane >> 4) + register
template <int TILES>
__device__ __forceinline__ void store_relu(const f32x4 (&acc)[TILES], const float* __restrict__ bias, int nt0, float* dst, int stride, int lane) {
  const int col = lane & 15, r0 = 4 * (lane >> 4);
#pragma unroll
  for (int t = 0; t < TILES; t++) {
    const float b = bias[16 * (nt0 + t) + col];
#pragma unroll
    for (int r = 0; r < 4; r++) dst[(r0 + r) * stride + 16 * (nt0 + t) + col] = fmaxf(acc[t][r] + b, 0.0f);
  }
}

// The critic's layer 0 of forward_kernel<kObs + kPriv>: 208 / 16 = 13 k-groups, which no pipeline depth above 1 divides.
// 1: twelve k-groups at depth 2 + the last one on its own (its weights are fetched behind the twelve);  0: all thirteen at depth 1 (no
// weight of the next k-group in flight during the MFMAs of the current one).  12 + 1 ships: MI355X, n = 4096, medians of 5 x 300
// alternated launches in one process (tools/diag/privileged_time.py --alt-policy-lib, profiles/privileged_critic.txt): the plain kernel
// 0.0364 ms, 12 + 1 0.0385 (+5.8 %; the 96 added MFMAs on 1728 per wave are +5.6 %), depth 1 0.0387 (+6.3 %).  Both give the same bits
// (the k-groups are accumulated in the same order).  The switch stays for that tool.
#ifndef ORR_POLICY_PRIV_SPLIT
#define ORR_POLICY_PRIV_SPLIT 1
#endif

// KV: the width of the critic's input.  kObs: actor and critic read the observation (orr_policy_forward).  kObs + kPriv: the critic's
// layer 0 reads the LDS tile obs | priv against a (kObs + kPriv) x 512 matrix (orr_policy_forward_priv); the actor reads the first kObs
// columns of the same tile with the same code, so its outputs are bit for bit the plain kernel's.
// KP: the width of the actor's input.  kObs + kPriv (orr_policy_forward_teacher, with KV = kObs + kPriv): the actor's layer 0 reads the whole
// tile too, against its own (kObs + kPriv) x 512 matrix, by the critic's k-groups (twelve at depth 2 + one).  That instantiation also takes
// value == NULL as "no critic": the test is on a kernel argument, i.e. uniform over the workgroup, it guards the critic's layers only and
// every barrier is outside it; the actor's instructions and inputs are the same either way, and so are action, raw and mean.
// HIST (orr_policy_forward_history, with KV = KP = kObs + kPriv): the privileged columns of the tile are not read but computed, by an encoder
// over the robot's sensor history, z = relu(hist W0 + b0) W1 + b1.  The history tile and the encoder's hidden layer use the LDS of the hidden
// layers before those are written; everything behind the tile is the teacher kernel's code on the same k-groups, hence its bits.  The kernel
// takes HistParams and calls layer<> with a UNIT of its own (KP + 1), so the three older instantiations keep their arguments and their code.
// HIST with KV = KP + kPriv (orr_policy_forward_history_priv): the asymmetric critic of a history policy.  The tile is obs | z | priv, KV words
// wide: the actor reads obs | z, the history kernel's code on the same k-groups, the critic reads obs | priv - the TRUE row, P.priv - against its
// (kObs + kPriv) x 512 matrix: k-groups 0..9 from the observation's columns, 10..12 from the row's behind z, accumulated in the teacher
// kernel's order (hence its value, bit for bit).  A UNIT of its own again (KP + 2).
template <int KV, int KP = kObs, bool HIST = false>
__global__ __launch_bounds__(256) void forward_kernel(typename std::conditional<HIST, HistParams, Params>::type P) {
  constexpr bool CPRIV = HIST && KV == KP + kPriv;
  constexpr int UNIT = HIST ? (CPRIV ? KP + 2 : KP + 1) : KP;
  static_assert(!HIST || (KP == kObs + kPriv && (KV == KP || CPRIV)), "the encoder fills the teacher's privileged columns");
  constexpr int kObsStride = KV + 1;            // odd strides: the 16 rows of an A fragment fall into distinct LDS banks
  static_assert(KV >= kObs && KV % 16 == 0 && (kObsStride & 1) == 1, "whole k-groups, odd stride");
  static_assert(KP == kObs || KP == KV || CPRIV, "the actor reads the observation or the critic's whole tile");
  static_assert((kRows * kObsStride + kRows * kH0Stride + kRows * kH1Stride) * sizeof(float) <= 160 * 1024, "static LDS beyond the 160 KB of a gfx950 CU");
  __shared__ float s_obs[kRows * kObsStride];
  __shared__ float s_h0[kRows * kH0Stride];
  __shared__ float s_h1[kRows * kH1Stride];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * kRows;
  // observation tile (rows beyond n read as zero)
  for (int i = tid; i < kRows * kObs; i += 256) {
    const int r = i / kObs, c = i - r * kObs;
    s_obs[r * kObsStride + c] = (row0 + r) < P.n ? P.obs[(size_t)(row0 + r) * kObs + c] : 0.0f;
  }
  if constexpr (HIST) {        // privileged columns behind it: the encoder's output
    const f32x4* h4 = reinterpret_cast<const f32x4*>(P.hist);
    for (int i = tid; i < kRows * (kHist / 4); i += 256) {
      const int r = i / (kHist / 4), c4 = i - r * (kHist / 4);
      const f32x4 v = (row0 + r) < P.n ? h4[(size_t)(row0 + r) * (kHist / 4) + c4] : f32x4{0, 0, 0, 0};
      float* d = s_h0 + r * kHistStride + 4 * c4;
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
    if constexpr (CPRIV) {     // the true row behind the estimate's columns, for the critic alone (no critic: P.priv may be NULL)
      if (P.value) {
        for (int i = tid; i < kRows * kPriv; i += 256) {
          const int r = i / kPriv, c = i - r * kPriv;
          s_obs[r * kObsStride + KP + c] = (row0 + r) < P.n ? P.priv[(size_t)(row0 + r) * kPriv + c] : 0.0f;
        }
      }
    }
    __syncthreads();
    {   // encoder layer 0: 512 -> 256; this wave: column tiles [4 wave, 4 wave + 4), the shape of layer 1 below
      f32x4 acc[4];
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = f32x4{0, 0, 0, 0};
      layer<UNIT, 4, kHist, 4>(acc, P.enc.w0, 4 * wave, s_h0, kHistStride, lane);
      store_relu<4>(acc, P.enc.b0, 4 * wave, s_h1, kH1Stride, lane);
    }
    __syncthreads();
    if (wave < kPriv / 16) {   // encoder layer 1: 256 -> 48, one column tile each on waves 0..2; no ReLU
      f32x4 acc[1] = {f32x4{0, 0, 0, 0}};
      layer<UNIT, 1, kEncH, 4>(acc, P.enc.w1, wave, s_h1, kH1Stride, lane);
      const int c = 16 * wave + (lane & 15), r0 = 4 * (lane >> 4);
      const float b = P.enc.b1[c];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float z = acc[0][r] + b;
        s_obs[(r0 + r) * kObsStride + kObs + c] = z;
        if (P.latent && row0 + r0 + r < P.n) P.latent[(size_t)(row0 + r0 + r) * kPriv + c] = z;
      }
    }
  } else if constexpr (KV > kObs) {   // privileged columns behind it
    constexpr int kP = KV - kObs;
    for (int i = tid; i < kRows * kP; i += 256) {
      const int r = i / kP, c = i - r * kP;
      s_obs[r * kObsStride + kObs + c] = (row0 + r) < P.n ? P.priv[(size_t)(row0 + r) * kP + c] : 0.0f;
    }
  }
  __syncthreads();
  // ---- layer 0: 160 -> 512, actor and critic; this wave: column tiles [8 wave, 8 wave + 8) of each ----
  {
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; t++) acc[t] = f32x4{0, 0, 0, 0};
    if constexpr (KP == kObs) {
      layer<UNIT, 8, kObs, 2>(acc, P.net.w0_pi, 8 * wave, s_obs, kObsStride, lane);
    } else {
      constexpr int kMain = KP / 32 * 32;
      layer<UNIT, 8, kMain, 2, KP / 16, 0>(acc, P.net.w0_pi, 8 * wave, s_obs, kObsStride, lane);
      layer<UNIT, 8, KP - kMain, 1, KP / 16, kMain / 16>(acc, P.net.w0_pi, 8 * wave, s_obs + kMain, kObsStride, lane);
    }
    store_relu<8>(acc, P.net.b0_pi, 8 * wave, s_h0, kH0Stride, lane);
    if (KP == kObs || P.value) {       // KP == kObs: a constant, no test in those two kernels
#pragma unroll
      for (int t = 0; t < 8; t++) acc[t] = f32x4{0, 0, 0, 0};
      if constexpr (CPRIV) {                      // the teacher kernel's order: twelve k-groups at depth 2 (ten of obs, two of priv), then one
        constexpr int kMain = KP / 32 * 32;
        layer<UNIT, 8, kObs, 2, KP / 16, 0>(acc, P.net.w0_vf, 8 * wave, s_obs, kObsStride, lane);
        layer<UNIT, 8, kMain - kObs, 2, KP / 16, kObs / 16>(acc, P.net.w0_vf, 8 * wave, s_obs + KP, kObsStride, lane);
        layer<UNIT, 8, KP - kMain, 1, KP / 16, kMain / 16>(acc, P.net.w0_vf, 8 * wave, s_obs + KP + (kMain - kObs), kObsStride, lane);
      } else if constexpr (KV == kObs) {
        layer<UNIT, 8, kObs, 2>(acc, P.net.w0_vf, 8 * wave, s_obs, kObsStride, lane);
      } else if constexpr (ORR_POLICY_PRIV_SPLIT) {
        constexpr int kMain = KV / 32 * 32;       // the k-groups that depth 2 divides
        layer<UNIT, 8, kMain, 2, KV / 16, 0>(acc, P.net.w0_vf, 8 * wave, s_obs, kObsStride, lane);
        layer<UNIT, 8, KV - kMain, 1, KV / 16, kMain / 16>(acc, P.net.w0_vf, 8 * wave, s_obs + kMain, kObsStride, lane);
      } else {
        layer<UNIT, 8, KV, 1>(acc, P.net.w0_vf, 8 * wave, s_obs, kObsStride, lane);
      }
      store_relu<8>(acc, P.net.b0_vf, 8 * wave, s_h0 + kH0, kH0Stride, lane);
    }
  }
  __syncthreads();
  // ---- layer 1: 512 -> 256; this wave: column tiles [4 wave, 4 wave + 4) of each net ----
  {
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = f32x4{0, 0, 0, 0};
    layer<UNIT, 4, kH0, 4>(acc, P.net.w1_pi, 4 * wave, s_h0, kH0Stride, lane);
    store_relu<4>(acc, P.net.b1_pi, 4 * wave, s_h1, kH1Stride, lane);
    if (KP == kObs || P.value) {
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = f32x4{0, 0, 0, 0};
      layer<UNIT, 4, kH0, 4>(acc, P.net.w1_vf, 4 * wave, s_h0 + kH0, kH0Stride, lane);
      store_relu<4>(acc, P.net.b1_vf, 4 * wave, s_h1 + kH1, kH1Stride, lane);
    }
  }
  __syncthreads();
  // ---- heads: wave 0 the actor (12 of 16 columns), wave 1 the critic (1 of 16 columns) ----
  if (wave >= 2) return;
  f32x4 acc[1] = {f32x4{0, 0, 0, 0}};
  const int col = lane & 15, r0 = 4 * (lane >> 4);
  if (wave == 0) {
    layer<UNIT, 1, kH1, 4>(acc, P.net.w2_pi, 0, s_h1, kH1Stride, lane);
    if (col < kAct) {
      const float b = P.net.b2_pi[col];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int robot = row0 + r0 + r;
        if (robot < P.n) {
          const size_t o = (size_t)robot * kAct + col;
          const float mu = acc[0][r] + b;
          const float a = P.noise ? mu + P.std * P.noise[o] : mu;
          P.action[o] = fminf(fmaxf(a, -P.clip), P.clip);
          if (P.raw) P.raw[o] = a;
          if (P.mean) P.mean[o] = mu;
        }
      }
    }
  } else if (KP == kObs || P.value) {
    layer<UNIT, 1, kH1, 4>(acc, P.net.w2_vf, 0, s_h1 + kH1, kH1Stride, lane);
    if (col == 0 && P.value) {
      const float b = P.net.b2_vf[0];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int robot = row0 + r0 + r;
        if (robot < P.n) P.value[robot] = acc[0][r] + b;
      }
    }
  }
}

// The sensor history's shift (orr_history_push).  A thread owns ONE 16-byte quad of the frame across all 16 slots of one robot: it loads its
// 15 quads prev[i][0..14][q] into registers, then stores next[i][1..15][q] and the new frame's quad - only to addresses of a column that it
// alone has loaded, so prev == next needs no barrier (which would not order one wave's loads against another's stores anyway).  prev and next
// carry no __restrict__ for that reason.  8 threads per robot, 32 robots per workgroup.
constexpr int kHistSteps = ORR_HISTORY_STEPS, kHistQuads = ORR_HISTORY_FRAME / 4;
static_assert(kHistSteps * kHistQuads * 4 == kHist && kHistQuads == 8, "16 slots of 8 quads");
__global__ __launch_bounds__(256) void history_push_kernel(const float* __restrict__ obs, const uint8_t* __restrict__ done, const float* prev,
                                                           float* next, int n) {
  const int i = blockIdx.x * (256 / kHistQuads) + threadIdx.x / kHistQuads, q = threadIdx.x % kHistQuads;
  if (i >= n) return;
  // quad 0: the IMU's newest reading obs[0:4]; 1..3: the last action obs[12:24]; 4..6: the motor angles obs[48:60]; 7: the pad
  f32x4 frame = {0, 0, 0, 0};
  if (q < 7) {
    const float* o = obs + (size_t)i * kObs + (q == 0 ? 0 : (q < 4 ? 12 + 4 * (q - 1) : 48 + 4 * (q - 4)));
    frame = f32x4{o[0], o[1], o[2], o[3]};
  }
  const bool fresh = done ? done[i] != 0 : true;
  const f32x4* p4 = reinterpret_cast<const f32x4*>(prev) + (size_t)i * (kHistSteps * kHistQuads) + q;
  f32x4* n4 = reinterpret_cast<f32x4*>(next) + (size_t)i * (kHistSteps * kHistQuads) + q;
  f32x4 h[kHistSteps - 1];
#pragma unroll
  for (int s = 0; s < kHistSteps - 1; s++) h[s] = frame;
  if (!fresh) {
#pragma unroll
    for (int s = 0; s < kHistSteps - 1; s++) h[s] = p4[s * kHistQuads];
  }
  n4[0] = frame;
#pragma unroll
  for (int s = 0; s < kHistSteps - 1; s++) n4[(s + 1) * kHistQuads] = h[s];
}

// One thread per robot: backward recursion over the segment, then mean / variance / standardisation of its own T values.
// legacy (ORR_GAE_LEGACY_INDEX): the recursion's "nonterminal" is read where the reference reads it, episode_starts[(step * N + i) + (1 + i)]
// of the flat [T * N] (+ N x False) array (agents/ppo_imitation.py:88) - robot i's own next-step flag only for N = 1, otherwise the flag of
// robot (2 i + 1) mod N at step t + (2 i + 1) / N.  episode_starts[t'][j] = done[t' - 1][j], and first_starts[j] for t' = 0.  The
// one-step value target still uses the robot's own flag (nextvpreds is filled per robot by the runner, imitation_runners.py:174-188).
__global__ void gae_kernel(const float* __restrict__ rewards, const float* __restrict__ vpred, const uint8_t* __restrict__ dones,
                           const uint8_t* __restrict__ first_starts, const float* __restrict__ bootstrap, int T, int N, float gamma,
                           float lam, int flags, float eps, float* __restrict__ adv, float* __restrict__ ret) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const bool normalize = flags & ORR_GAE_NORMALIZE, legacy = flags & ORR_GAE_LEGACY_INDEX;
  float last = 0.0f, next_v = bootstrap ? bootstrap[n] : 0.0f, sum = 0.0f;
  for (int k = T - 1; k >= 0; k--) {
    const size_t o = (size_t)k * N + n;
    const float own = dones[o] ? 0.0f : 1.0f, v = vpred[o];
    float nonterminal = own;
    if (legacy) {
      const long long f = (long long)k * N + 2 * n + 1;
      const int ts = (int)(f / N), js = (int)(f % N);
      const bool start = ts >= T ? false : (ts == 0 ? (first_starts ? first_starts[js] != 0 : true) : dones[(size_t)(ts - 1) * N + js] != 0);
      nonterminal = start ? 0.0f : 1.0f;
    }
    const float delta = rewards[o] + gamma * next_v * own - v;
    last = delta + gamma * lam * nonterminal * last;
    adv[o] = last;
    ret[o] = last + v;
    sum += last;
    next_v = v;
  }
  if (!normalize) return;
  const float mean = sum / (float)T;
  float var = 0.0f;
  for (int k = 0; k < T; k++) { const float d = adv[(size_t)k * N + n] - mean; var += d * d; }
  const float inv = 1.0f / (sqrtf(var / (float)T) + eps);
  for (int k = 0; k < T; k++) { const size_t o = (size_t)k * N + n; adv[o] = (adv[o] - mean) * inv; }
}

// ---- orr_history_student_head (include/openroborl_learner.h): the action loss of a history student through the frozen actor ----------------
// Forward, loss and backward to the latent for a tile of 16 samples in one launch, the forward kernel's mapping: four waves, the tile
// obs | z and both hidden layers in LDS, weights streamed in orr_policy_pack's fragments.  The forward layers are forward_kernel<208, 208>'s
// calls on the same k-groups (hence the teacher kernel's mean, bit for bit); the backward layers are layer<> again, against the packed
// transposes: g_h1 = g_mean W2^T (K = 16: the 12 actions + 4 zero columns), g_h0 = g_h1 W1^T (K = 256), g_z = g_h0 W0[160:208]^T (K = 512,
// one column tile on each of three waves).  A masked gradient overwrites the activation it masks (h > 0, orr_relu_backward's convention):
// a lane reads and writes the four C-layout elements that it owns, and no other lane touches them between the two barriers around a layer.
// No weight gradient: the actor is frozen.  MFMAs per wave: 416 + 512 + 64 forward, 16 + 512 + 128 backward = 1648.
// Its own UNIT for layer<> (see there): the forward kernels share no instantiation with it.
struct HeadParams {
  const float *w0, *b0, *w1, *b1, *w2, *b2;    // orr_policy_net's actor
  const float *w2t, *w1t, *w0zt;               // the packed transposes
  const float *obs, *z, *target_mean, *target_priv;
  float *g_z, *mean, *partials;
  int m, nblk;
  float g_act, g_lat, inv_m;                   // 2 action_coef / m, 2 latent_coef / m, 1 / m
};
constexpr int kHeadUnit = 2 * (kObs + kPriv);
constexpr int kInStride = kObs + kPriv + 1, kG0Stride = kH0 + 1, kG1Stride = kH1 + 1, kGmStride = 17;    // odd, like the forward kernel's tiles
static_assert(kInStride % 2 == 1 && kG0Stride % 2 == 1 && kG1Stride % 2 == 1 && kGmStride % 2 == 1, "odd LDS strides");

// store_relu's text under a name of this kernel's own, for the reason layer<> takes a UNIT: a fifth caller of store_relu<8> and <4> changed
// the four forward kernels' instructions (profiles/history_action_loss.txt)
template <int TILES>
__device__ __forceinline__ void head_store_relu(const f32x4 (&acc)[TILES], const float* __restrict__ bias, int nt0, float* dst, int stride, int lane) {
  const int col = lane & 15, r0 = 4 * (lane >> 4);
#pragma unroll
  for (int t = 0; t < TILES; t++) {
    const float b = bias[16 * (nt0 + t) + col];
#pragma unroll
    for (int r = 0; r < 4; r++) dst[(r0 + r) * stride + 16 * (nt0 + t) + col] = fmaxf(acc[t][r] + b, 0.0f);
  }
}

template <int TILES>
__device__ __forceinline__ void store_masked(const f32x4 (&acc)[TILES], int nt0, float* h, int stride, int lane) {
  const int col = lane & 15, r0 = 4 * (lane >> 4);
#pragma unroll
  for (int t = 0; t < TILES; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      float* p = h + (r0 + r) * stride + 16 * (nt0 + t) + col;
      *p = *p > 0.0f ? acc[t][r] : 0.0f;
    }
}

__device__ __forceinline__ float head_wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  return x;
}

__global__ __launch_bounds__(256) void student_head_kernel(HeadParams P) {
  constexpr int UNIT = kHeadUnit, KP = kObs + kPriv, kMain = KP / 32 * 32;
  __shared__ float s_in[kRows * kInStride];
  __shared__ float s_h0[kRows * kG0Stride];
  __shared__ float s_h1[kRows * kG1Stride];
  __shared__ float s_gm[kRows * kGmStride];
  __shared__ float s_loss[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * kRows;
  const int col = lane & 15, r0 = 4 * (lane >> 4);
  // the tile obs | z (rows beyond m read as zero)
  for (int i = tid; i < kRows * kObs; i += 256) {
    const int r = i / kObs, c = i - r * kObs;
    s_in[r * kInStride + c] = (row0 + r) < P.m ? P.obs[(size_t)(row0 + r) * kObs + c] : 0.0f;
  }
  for (int i = tid; i < kRows * kPriv; i += 256) {
    const int r = i / kPriv, c = i - r * kPriv;
    s_in[r * kInStride + kObs + c] = (row0 + r) < P.m ? P.z[(size_t)(row0 + r) * kPriv + c] : 0.0f;
  }
  __syncthreads();
  // ---- forward: the teacher kernel's actor ----
  {
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; t++) acc[t] = f32x4{0, 0, 0, 0};
    layer<UNIT, 8, kMain, 2, KP / 16, 0>(acc, P.w0, 8 * wave, s_in, kInStride, lane);
    layer<UNIT, 8, KP - kMain, 1, KP / 16, kMain / 16>(acc, P.w0, 8 * wave, s_in + kMain, kInStride, lane);
    head_store_relu<8>(acc, P.b0, 8 * wave, s_h0, kG0Stride, lane);
  }
  __syncthreads();
  {
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = f32x4{0, 0, 0, 0};
    layer<UNIT, 4, kH0, 4>(acc, P.w1, 4 * wave, s_h0, kG0Stride, lane);
    head_store_relu<4>(acc, P.b1, 4 * wave, s_h1, kG1Stride, lane);
  }
  __syncthreads();
  // ---- the head and the action loss on wave 0: g_mean = 2 action_coef (mean - target) / m, a 16 x 16 tile with columns 12..15 zero ----
  if (wave == 0) {
    f32x4 acc[1] = {f32x4{0, 0, 0, 0}};
    layer<UNIT, 1, kH1, 4>(acc, P.w2, 0, s_h1, kG1Stride, lane);
    const float b = col < kAct ? P.b2[col] : 0.0f;
    float sq = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = row0 + r0 + r;
      float gm = 0.0f;
      if (col < kAct && row < P.m) {
        const size_t o = (size_t)row * kAct + col;
        const float mu = acc[0][r] + b;
        if (P.mean) P.mean[o] = mu;
        const float d = mu - P.target_mean[o];
        gm = P.g_act * d;
        sq += d * d;
      }
      s_gm[(r0 + r) * kGmStride + col] = gm;
    }
    sq = head_wave_sum(sq);
    if (lane == 0) s_loss[0] = sq;
  }
  __syncthreads();
  // ---- backward: 12 (16) -> 256, masked by h1 > 0, over h1 ----
  {
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = f32x4{0, 0, 0, 0};
    layer<UNIT, 4, 16, 1>(acc, P.w2t, 4 * wave, s_gm, kGmStride, lane);
    store_masked<4>(acc, 4 * wave, s_h1, kG1Stride, lane);
  }
  __syncthreads();
  // ---- 256 -> 512, masked by h0 > 0, over h0 ----
  {
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; t++) acc[t] = f32x4{0, 0, 0, 0};
    layer<UNIT, 8, kH1, 2>(acc, P.w1t, 8 * wave, s_h1, kG1Stride, lane);
    store_masked<8>(acc, 8 * wave, s_h0, kG0Stride, lane);
  }
  __syncthreads();
  // ---- 512 -> 48 on three waves, + the latent loss's own gradient; column sums and loss shares of the tile ----
  if (wave < kPriv / 16) {
    f32x4 acc[1] = {f32x4{0, 0, 0, 0}};
    layer<UNIT, 1, kH0, 4>(acc, P.w0zt, wave, s_h0, kG0Stride, lane);
    const int c = 16 * wave + col;
    float cs = 0.0f, sq = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = row0 + r0 + r;
      if (row < P.m) {
        const size_t o = (size_t)row * kPriv + c;
        const float d = s_in[(r0 + r) * kInStride + kObs + c] - P.target_priv[o];
        const float g = acc[0][r] + P.g_lat * d;
        P.g_z[o] = g;
        cs += g;
        sq += d * d;
      }
    }
    cs += __shfl_xor(cs, 16, 64);     // the four row groups of a column, in a fixed order
    cs += __shfl_xor(cs, 32, 64);
    if (lane < 16) P.partials[(size_t)blockIdx.x * kPriv + c] = cs;
    sq = head_wave_sum(sq);
    if (lane == 0) s_loss[1 + wave] = sq;
  }
  __syncthreads();
  if (tid == 0) {
    float* loss = P.partials + (size_t)P.nblk * kPriv + 2 * (size_t)blockIdx.x;
    loss[0] = s_loss[0] * P.inv_m;
    loss[1] = ((s_loss[1] + s_loss[2]) + s_loss[3]) * P.inv_m;
  }
}

// ---- orr_latent_backward (include/openroborl_learner.h): the PPO gradient from the actor's layer 0 into a history policy's latent ------------
// The last stage of student_head_kernel as a launch of its own: a workgroup owns 16 samples, their g0 tile [16][512] goes to LDS, and waves
// 0..2 each form one 16-column tile of g_z = g0 W0[160:208]^T (K = 512: 128 MFMAs, a k-ordered chain per element, so a row's bits do not
// depend on m), add the latent loss's own gradient, and leave the tile's column sums and its share of the loss.  latent_coef == 0 reaches the
// kernel as a NULL z, a test on a kernel argument: z and target_priv are then not read.  Its own UNIT for layer<>, like every kernel of this file.
struct LatentParams {
  const float *g0, *w0zt, *z, *target_priv;
  float *g_z, *partials;
  int m, nblk;
  float g_lat;                                 // 2 latent_coef / m
};
constexpr int kLatentUnit = kHeadUnit + 1;

__global__ __launch_bounds__(256) void latent_backward_kernel(LatentParams P) {
  __shared__ float s_g[kRows * kG0Stride];
  __shared__ double s_loss[kPriv / 16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * kRows;
  for (int i = tid; i < kRows * kH0; i += 256) {      // rows beyond m read as zero
    const int r = i / kH0, c = i - r * kH0;
    s_g[r * kG0Stride + c] = (row0 + r) < P.m ? P.g0[(size_t)(row0 + r) * kH0 + c] : 0.0f;
  }
  __syncthreads();
  if (wave < kPriv / 16) {
    f32x4 acc[1] = {f32x4{0, 0, 0, 0}};
    layer<kLatentUnit, 1, kH0, 4>(acc, P.w0zt, wave, s_g, kG0Stride, lane);
    const int c = 16 * wave + (lane & 15), r0 = 4 * (lane >> 4);
    const bool latent = P.z != nullptr;        // NULL with latent_coef == 0 (the host function sees to it)
    float cs = 0.0f;
    double sq = 0.0;                           // the tile's 768 squares in float64 (exact differences): the share is rounded once, on its way out
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = row0 + r0 + r;
      if (row < P.m) {
        const size_t o = (size_t)row * kPriv + c;
        float g = acc[0][r];
        if (latent) {
          const float zv = P.z[o], tv = P.target_priv[o];
          const double d = (double)zv - (double)tv;
          g += P.g_lat * (zv - tv);
          sq += d * d;
        }
        P.g_z[o] = g;
        cs += g;
      }
    }
    cs += __shfl_xor(cs, 16, 64);     // the four row groups of a column, in a fixed order
    cs += __shfl_xor(cs, 32, 64);
    if (lane < 16) P.partials[(size_t)blockIdx.x * kPriv + c] = cs;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_down(sq, o, 64);
    if (lane == 0) s_loss[wave] = sq;
  }
  __syncthreads();
  if (tid == 0) P.partials[(size_t)P.nblk * kPriv + blockIdx.x] = (float)(((s_loss[0] + s_loss[1]) + s_loss[2]) / (double)P.m);
}

}  // namespace

extern "C" {

int64_t orr_policy_packed_size(int32_t k, int32_t n) {
  if (k <= 0 || n <= 0 || (k % 16) != 0) return -1;
  return (int64_t)((n + 15) / 16) * (k / 16) * 256;
}

int32_t orr_policy_pack(const float* w_dev, int32_t k, int32_t n, float* out_dev, void* stream) {
  const long long total = orr_policy_packed_size(k, n);
  if (!w_dev || !out_dev || total < 0) return orr_fail(-1, "orr_policy_pack: bad argument (K must be a multiple of 16)", hipSuccess);
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_dev, (int)k, (int)n, out_dev, total);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_policy_pack: launch", e);
  return 0;
}

int32_t orr_policy_pack_norm(const float* w_dev, int32_t k, int32_t n, const float* mean, const float* rstd, const float* b, float* out_dev,
                             float* out_b, void* stream) {
  const long long total = orr_policy_packed_size(k, n);
  if (!w_dev || !out_dev || total < 0) return orr_fail(-1, "orr_policy_pack_norm: bad argument (K must be a multiple of 16)", hipSuccess);
  if (!mean || !rstd || !b || !out_b) return orr_fail(-1, "orr_policy_pack_norm: null statistics table or bias", hipSuccess);
  if ((reinterpret_cast<uintptr_t>(mean) & 15) || (reinterpret_cast<uintptr_t>(rstd) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
    return orr_fail(-1, "orr_policy_pack_norm: mean, rstd and the packed image must be 16-byte aligned", hipSuccess);
  if ((reinterpret_cast<uintptr_t>(w_dev) & 3) || (reinterpret_cast<uintptr_t>(b) & 3) || (reinterpret_cast<uintptr_t>(out_b) & 3))
    return orr_fail(-1, "orr_policy_pack_norm: w, b and out_b must be 4-byte aligned", hipSuccess);
  const int pack_blocks = (int)((total + 255) / 256), bias_blocks = (n + 255) / 256;
  hipLaunchKernelGGL(pack_norm_kernel, dim3((unsigned)(pack_blocks + bias_blocks)), dim3(256), 0, (hipStream_t)stream, w_dev, (int)k, (int)n, mean, rstd,
                     b, out_dev, out_b, total, pack_blocks);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_policy_pack_norm: launch", e);
  return 0;
}

int32_t orr_policy_forward(const orr_policy_net* net, const float* obs, int32_t n, const float* noise, float std, float clip,
                           float* action, float* raw, float* value, float* mean, void* stream) {
  if (!net || !obs || !action || n < 0) return orr_fail(-1, "orr_policy_forward: bad argument", hipSuccess);
  const float* const* p = reinterpret_cast<const float* const*>(net);
  for (int i = 0; i < 12; i++)
    if (!p[i]) return orr_fail(-1, "orr_policy_forward: orr_policy_net has a null pointer", hipSuccess);
  if (n == 0) return 0;
  Params P;
  P.net = *net; P.obs = obs; P.noise = noise; P.action = action; P.raw = raw; P.value = value; P.mean = mean;
  P.n = n; P.std = std; P.clip = clip; P.priv = nullptr;
  hipLaunchKernelGGL(forward_kernel<kObs>, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(256), 0, (hipStream_t)stream, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_policy_forward: launch", e);
  return 0;
}

int32_t orr_policy_forward_priv(const orr_policy_net* net, const float* obs, const float* priv, int32_t n, const float* noise, float std, float clip,
                                float* action, float* raw, float* value, float* mean, void* stream) {
  if (!net || !obs || !priv || !action || n < 0) return orr_fail(-1, "orr_policy_forward_priv: bad argument", hipSuccess);
  const float* const* p = reinterpret_cast<const float* const*>(net);
  for (int i = 0; i < 12; i++)
    if (!p[i]) return orr_fail(-1, "orr_policy_forward_priv: orr_policy_net has a null pointer", hipSuccess);
  if (n == 0) return 0;
  Params P;
  P.net = *net; P.obs = obs; P.noise = noise; P.action = action; P.raw = raw; P.value = value; P.mean = mean;
  P.n = n; P.std = std; P.clip = clip; P.priv = priv;
  hipLaunchKernelGGL(forward_kernel<kObs + kPriv>, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(256), 0, (hipStream_t)stream, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_policy_forward_priv: launch", e);
  return 0;
}

int32_t orr_policy_forward_teacher(const orr_policy_net* net, const float* obs, const float* priv, int32_t n, const float* noise, float std,
                                   float clip, float* action, float* raw, float* value, float* mean, void* stream) {
  if (!net || !obs || !priv || !action || n <= 0) return orr_fail(-1, "orr_policy_forward_teacher: bad argument", hipSuccess);
  const float* const* p = reinterpret_cast<const float* const*>(net);
  for (int i = 0; i < 12; i++) {
    if (!p[i]) return orr_fail(-1, "orr_policy_forward_teacher: orr_policy_net has a null pointer", hipSuccess);
    if (reinterpret_cast<uintptr_t>(p[i]) & (i % 2 == 0 ? 15 : 3))     // packed weights are read 16 bytes per lane
      return orr_fail(-1, "orr_policy_forward_teacher: packed weights must be 16-byte aligned, biases 4-byte aligned", hipSuccess);
  }
  for (const void* q : {(const void*)obs, (const void*)priv, (const void*)noise, (const void*)action, (const void*)raw, (const void*)value, (const void*)mean})
    if (reinterpret_cast<uintptr_t>(q) & 3) return orr_fail(-1, "orr_policy_forward_teacher: buffers must be 4-byte aligned", hipSuccess);
  Params P;
  P.net = *net; P.obs = obs; P.noise = noise; P.action = action; P.raw = raw; P.value = value; P.mean = mean;
  P.n = n; P.std = std; P.clip = clip; P.priv = priv;
  hipLaunchKernelGGL((forward_kernel<kObs + kPriv, kObs + kPriv>), dim3((unsigned)((n + kRows - 1) / kRows)), dim3(256), 0, (hipStream_t)stream, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_policy_forward_teacher: launch", e);
  return 0;
}

int32_t orr_policy_forward_history(const orr_policy_net* net, const orr_history_encoder* enc, const float* obs, const float* hist, int32_t n,
                                   const float* noise, float std, float clip, float* action, float* raw, float* value, float* mean,
                                   float* latent, void* stream) {
  if (!net || !enc || !obs || !hist || !action || n <= 0) return orr_fail(-1, "orr_policy_forward_history: bad argument", hipSuccess);
  const float* const* p = reinterpret_cast<const float* const*>(net);
  for (int i = 0; i < 12; i++) {
    if (!p[i]) return orr_fail(-1, "orr_policy_forward_history: orr_policy_net has a null pointer", hipSuccess);
    if (reinterpret_cast<uintptr_t>(p[i]) & (i % 2 == 0 ? 15 : 3))     // packed weights are read 16 bytes per lane
      return orr_fail(-1, "orr_policy_forward_history: packed weights must be 16-byte aligned, biases 4-byte aligned", hipSuccess);
  }
  const float* const* q = reinterpret_cast<const float* const*>(enc);
  for (int i = 0; i < 4; i++) {
    if (!q[i]) return orr_fail(-1, "orr_policy_forward_history: orr_history_encoder has a null pointer", hipSuccess);
    if (reinterpret_cast<uintptr_t>(q[i]) & (i % 2 == 0 ? 15 : 3))
      return orr_fail(-1, "orr_policy_forward_history: packed weights must be 16-byte aligned, biases 4-byte aligned", hipSuccess);
  }
  if (reinterpret_cast<uintptr_t>(hist) & 15) return orr_fail(-1, "orr_policy_forward_history: hist must be 16-byte aligned", hipSuccess);
  for (const void* b : {(const void*)obs, (const void*)noise, (const void*)action, (const void*)raw, (const void*)value, (const void*)mean, (const void*)latent})
    if (reinterpret_cast<uintptr_t>(b) & 3) return orr_fail(-1, "orr_policy_forward_history: buffers must be 4-byte aligned", hipSuccess);
  HistParams P;
  P.net = *net; P.obs = obs; P.noise = noise; P.action = action; P.raw = raw; P.value = value; P.mean = mean;
  P.n = n; P.std = std; P.clip = clip; P.priv = nullptr;
  P.enc = *enc; P.hist = hist; P.latent = latent;
  hipLaunchKernelGGL((forward_kernel<kObs + kPriv, kObs + kPriv, true>), dim3((unsigned)((n + kRows - 1) / kRows)), dim3(256), 0, (hipStream_t)stream, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_policy_forward_history: launch", e);
  return 0;
}

int32_t orr_policy_forward_history_priv(const orr_policy_net* net, const orr_history_encoder* enc, const float* obs, const float* hist,
                                        const float* priv, int32_t n, const float* noise, float std, float clip, float* action, float* raw,
                                        float* value, float* mean, float* latent, void* stream) {
  if (!net || !enc || !obs || !hist || !action || n <= 0 || (value && !priv))
    return orr_fail(-1, "orr_policy_forward_history_priv: bad argument", hipSuccess);
  const float* const* p = reinterpret_cast<const float* const*>(net);
  for (int i = 0; i < 12; i++) {
    if (!p[i]) return orr_fail(-1, "orr_policy_forward_history_priv: orr_policy_net has a null pointer", hipSuccess);
    if (reinterpret_cast<uintptr_t>(p[i]) & (i % 2 == 0 ? 15 : 3))     // packed weights are read 16 bytes per lane
      return orr_fail(-1, "orr_policy_forward_history_priv: packed weights must be 16-byte aligned, biases 4-byte aligned", hipSuccess);
  }
  const float* const* q = reinterpret_cast<const float* const*>(enc);
  for (int i = 0; i < 4; i++) {
    if (!q[i]) return orr_fail(-1, "orr_policy_forward_history_priv: orr_history_encoder has a null pointer", hipSuccess);
    if (reinterpret_cast<uintptr_t>(q[i]) & (i % 2 == 0 ? 15 : 3))
      return orr_fail(-1, "orr_policy_forward_history_priv: packed weights must be 16-byte aligned, biases 4-byte aligned", hipSuccess);
  }
  if (reinterpret_cast<uintptr_t>(hist) & 15) return orr_fail(-1, "orr_policy_forward_history_priv: hist must be 16-byte aligned", hipSuccess);
  for (const void* b : {(const void*)obs, (const void*)priv, (const void*)noise, (const void*)action, (const void*)raw, (const void*)value,
                        (const void*)mean, (const void*)latent})
    if (reinterpret_cast<uintptr_t>(b) & 3) return orr_fail(-1, "orr_policy_forward_history_priv: buffers must be 4-byte aligned", hipSuccess);
  HistParams P;
  P.net = *net; P.obs = obs; P.noise = noise; P.action = action; P.raw = raw; P.value = value; P.mean = mean;
  P.n = n; P.std = std; P.clip = clip; P.priv = priv;
  P.enc = *enc; P.hist = hist; P.latent = latent;
  hipLaunchKernelGGL((forward_kernel<kObs + 2 * kPriv, kObs + kPriv, true>), dim3((unsigned)((n + kRows - 1) / kRows)), dim3(256), 0, (hipStream_t)stream, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_policy_forward_history_priv: launch", e);
  return 0;
}

int32_t orr_history_push(const float* obs, const uint8_t* done, const float* prev, float* next, int32_t n, void* stream) {
  if (!obs || !next || n <= 0 || (done && !prev)) return orr_fail(-1, "orr_history_push: bad argument", hipSuccess);
  if ((reinterpret_cast<uintptr_t>(prev) & 15) || (reinterpret_cast<uintptr_t>(next) & 15) || (reinterpret_cast<uintptr_t>(obs) & 3))
    return orr_fail(-1, "orr_history_push: prev and next must be 16-byte aligned, obs 4-byte aligned", hipSuccess);
  const uintptr_t a = reinterpret_cast<uintptr_t>(prev), b = reinterpret_cast<uintptr_t>(next), bytes = (uintptr_t)n * kHist * sizeof(float);
  if (prev && a != b && a < b + bytes && b < a + bytes)
    return orr_fail(-1, "orr_history_push: prev and next overlap without being equal", hipSuccess);
  hipLaunchKernelGGL(history_push_kernel, dim3((unsigned)((n + 256 / kHistQuads - 1) / (256 / kHistQuads))), dim3(256), 0, (hipStream_t)stream, obs,
                     done, prev, next, (int)n);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_history_push: launch", e);
  return 0;
}

int32_t orr_history_student_head(const orr_policy_net* net, const float* w2t, const float* w1t, const float* w0zt, const float* obs, const float* z,
                                 const float* target_mean, const float* target_priv, int32_t m, float action_coef, float latent_coef, float* g_z,
                                 float* mean, float* partials, void* stream) {
  if (!net || !w2t || !w1t || !w0zt || !obs || !z || !target_mean || !target_priv || !g_z || !partials || m <= 0)
    return orr_fail(-1, "orr_history_student_head: bad argument", hipSuccess);
  const float* const* p = reinterpret_cast<const float* const*>(net);
  for (int i = 0; i < 6; i++) {           // the actor's members only: the critic's are not read
    if (!p[i]) return orr_fail(-1, "orr_history_student_head: orr_policy_net's actor has a null pointer", hipSuccess);
    if (reinterpret_cast<uintptr_t>(p[i]) & (i % 2 == 0 ? 15 : 3))     // packed weights are read 16 bytes per lane
      return orr_fail(-1, "orr_history_student_head: packed weights must be 16-byte aligned, biases 4-byte aligned", hipSuccess);
  }
  for (const void* q : {(const void*)w2t, (const void*)w1t, (const void*)w0zt})
    if (reinterpret_cast<uintptr_t>(q) & 15) return orr_fail(-1, "orr_history_student_head: packed weights must be 16-byte aligned", hipSuccess);
  for (const void* q : {(const void*)obs, (const void*)z, (const void*)target_mean, (const void*)target_priv, (const void*)g_z, (const void*)mean,
                        (const void*)partials})
    if (reinterpret_cast<uintptr_t>(q) & 3) return orr_fail(-1, "orr_history_student_head: buffers must be 4-byte aligned", hipSuccess);
  HeadParams P;
  P.w0 = net->w0_pi; P.b0 = net->b0_pi; P.w1 = net->w1_pi; P.b1 = net->b1_pi; P.w2 = net->w2_pi; P.b2 = net->b2_pi;
  P.w2t = w2t; P.w1t = w1t; P.w0zt = w0zt;
  P.obs = obs; P.z = z; P.target_mean = target_mean; P.target_priv = target_priv;
  P.g_z = g_z; P.mean = mean; P.partials = partials;
  P.m = m; P.nblk = ORR_STUDENT_HEAD_ROWS(m);
  P.inv_m = 1.0f / (float)m; P.g_act = 2.0f * action_coef / (float)m; P.g_lat = 2.0f * latent_coef / (float)m;
  hipLaunchKernelGGL(student_head_kernel, dim3((unsigned)P.nblk), dim3(256), 0, (hipStream_t)stream, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_history_student_head: launch", e);
  return 0;
}

int32_t orr_latent_backward(const float* g0, const float* w0zt, const float* z, const float* target_priv, int32_t m, float latent_coef,
                            float* g_z, float* partials, void* stream) {
  if (!g0 || !w0zt || !g_z || !partials || m <= 0 || (latent_coef != 0.0f && (!z || !target_priv)))
    return orr_fail(-1, "orr_latent_backward: bad argument", hipSuccess);
  if (reinterpret_cast<uintptr_t>(w0zt) & 15) return orr_fail(-1, "orr_latent_backward: packed weights must be 16-byte aligned", hipSuccess);
  for (const void* q : {(const void*)g0, (const void*)z, (const void*)target_priv, (const void*)g_z, (const void*)partials})
    if (reinterpret_cast<uintptr_t>(q) & 3) return orr_fail(-1, "orr_latent_backward: buffers must be 4-byte aligned", hipSuccess);
  LatentParams P;
  P.g0 = g0; P.w0zt = w0zt; P.z = latent_coef != 0.0f ? z : nullptr; P.target_priv = latent_coef != 0.0f ? target_priv : nullptr; P.g_z = g_z; P.partials = partials;
  P.m = m; P.nblk = ORR_LATENT_BACKWARD_ROWS(m);
  P.g_lat = 2.0f * latent_coef / (float)m;
  hipLaunchKernelGGL(latent_backward_kernel, dim3((unsigned)P.nblk), dim3(256), 0, (hipStream_t)stream, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_latent_backward: launch", e);
  return 0;
}

int32_t orr_gae_flags(const float* rewards, const float* vpred, const uint8_t* dones, const uint8_t* first_starts, const float* bootstrap,
                      int32_t t, int32_t n, float gamma, float lam, int32_t flags, float eps, float* adv, float* ret, void* stream) {
  if (!rewards || !vpred || !dones || !adv || !ret || t <= 0 || n < 0) return orr_fail(-1, "orr_gae: bad argument", hipSuccess);
  if (flags & ~(ORR_GAE_NORMALIZE | ORR_GAE_LEGACY_INDEX)) return orr_fail(-1, "orr_gae: unknown flag", hipSuccess);
  if (n == 0) return 0;
  hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rewards, vpred, dones, first_starts,
                     bootstrap, (int)t, (int)n, gamma, lam, (int)flags, eps, adv, ret);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_gae: launch", e);
  return 0;
}

int32_t orr_gae(const float* rewards, const float* vpred, const uint8_t* dones, const float* bootstrap, int32_t t, int32_t n,
                float gamma, float lam, int32_t normalize, float eps, float* adv, float* ret, void* stream) {
  return orr_gae_flags(rewards, vpred, dones, nullptr, bootstrap, t, n, gamma, lam, normalize ? ORR_GAE_NORMALIZE : 0, eps, adv, ret, stream);
}

}  // extern "C"
