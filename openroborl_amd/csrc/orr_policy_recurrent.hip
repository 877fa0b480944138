// orr_policy_recurrent.hip -- one policy step of a RECURRENT policy in one launch (include/openroborl_policy.h: orr_policy_forward_recurrent):
// the GRU step of orr_recurrent.hip and the teacher-shaped actor / critic of orr_policy.hip, with an optional ASYMMETRIC critic.
//
//   h'  = start ? 0 : h0                                     x = obs[0:4] | obs[12:24] | obs[48:60] | 0 0 0 0
//   r   = sigmoid(x Wx_r + h' Wh_r + bx_r + bh_r)            u = sigmoid(x Wx_u + h' Wh_u + bx_u + bh_u)
//   q   = h' Wh_c + bh_c                                     c = tanh(x Wx_c + bx_c + r q)
//   h   = (1 - u) c + u h'                                   z = h Wo + bo
//   mean   = actor(obs | z)                                  action = clip(mean + std noise)
//   value  = critic(obs | priv)   with a priv,               critic(obs | z)   without one
//
// Mapping (that of both parent kernels): a workgroup of 256 threads (four waves, one per SIMD) owns 16 robots, the 16 rows of every
// matrix-core tile; 4096 robots are one workgroup per CU.  Every contraction is v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain per element)
// against orr_policy_pack's fragment-major images streamed from L2, one 16-byte load per lane and tile for four k-steps.
//
// LDS: ONE input tile of 16 x 256 words (stride 257), obs | z | priv, and the two hidden tiles of the MLPs (16 x 1024 and 16 x 512, odd
// strides).  Before the MLPs need them the hidden tiles hold the recurrence: h' (start mask applied on the way in) where hidden 0 will be,
// h where hidden 1 will be.
//   1. obs -> tile columns 0..159, h' -> the hidden-0 LDS, priv -> columns 208..255                                           barrier
//   2. gates, per wave: hidden units 64 w .. 64 w + 63 of r, u and c (column tiles 4 w .. 4 w + 3 of each gate), so that a lane holds r, u, q
//      and the x-part of c of the SAME (robot, unit) in the accumulators' C layout and combines them in registers.  The frame is not a tile
//      of its own: a lane's eight A words of the K = 32 contraction are read from the observation's columns of the input tile (the pad is a
//      literal zero).  K = 32 over x, then K = 256 over h', one accumulator per pre-activation.  h -> the hidden-1 LDS and hid             barrier
//   3. z on waves 0..2, one 16-column tile each (K = 256) -> tile columns 160..207 and latent                                      barrier
//   4. layer 0 of the actor over columns 0..207 (13 k-groups: twelve at depth 2 + one) and of the critic over obs | priv (columns 0..159 and
//      208..255, the same 13 k-groups of its matrix) or over obs | z -> hidden 0 (h' is dead since the barrier of 2)               barrier
//   5. layer 1 of both -> hidden 1 (h is dead since the barrier of 3)                                                              barrier
//   6. the heads: wave 0 the actor's with the Gaussian sample, wave 1 the critic's
// A barrier stands only where an LDS tile changes owner.  Every accumulator runs over k ascending from +0, in the order of orr_gru_forward and
// of orr_policy_forward_teacher, whose arithmetic outside the matrix cores is repeated here expression by expression: hid and latent are
// orr_gru_forward(T = 1)'s values, mean / action / raw orr_policy_forward_teacher(priv = z)'s and value its value on the critic's input.  A
// row's bits depend on neither n nor its neighbours.  Rows at or beyond n read as zero, count as started and write nothing.  No atomics.
//
// The helpers are this file's own (anonymous namespace): orr_policy.hip and orr_recurrent.hip share theirs with nobody, see layer<>'s UNIT there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/openroborl_policy.h"

int orr_fail(int code, const char* msg, hipError_t e);  // orr_kernels.hip

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kObs = ORR_POLICY_OBS_DIM, kH0 = ORR_POLICY_H0, kH1 = ORR_POLICY_H1, kAct = ORR_POLICY_ACT_DIM, kPriv = ORR_POLICY_PRIV_DIM;
constexpr int kFrame = ORR_HISTORY_FRAME, kHid = ORR_GRU_HIDDEN, kGates = ORR_GRU_GATES;
constexpr int kRows = 16;                                // robots per workgroup
constexpr int kIn = kObs + 2 * kPriv;                    // the input tile: obs | z | priv
constexpr int kNet = kObs + kPriv;                       // what a layer 0 reads
constexpr int kInStride = kIn + 1, kH0Stride = 2 * kH0 + 1, kH1Stride = 2 * kH1 + 1, kHStride = kHid + 1;   // odd: an A fragment's 16 rows in distinct banks
static_assert(kHid == 256 && kGates == 3 * kHid && kFrame == 32 && kPriv == 48 && kNet % 16 == 0, "four waves x four column tiles per gate; whole k-groups");
static_assert(kHStride <= kH0Stride && kHStride <= kH1Stride, "h' and h fit the hidden layers' LDS");
static_assert((kRows * kInStride + kRows * kH0Stride + kRows * kH1Stride) * sizeof(float) <= 160 * 1024, "static LDS beyond the 160 KB of a gfx950 CU");

// acc[s] += A(16 x 16 KG, from LDS) * B(tile(s), k-groups [G0, G0 + KG) of a packed matrix of KTOT k-groups) for NT column tiles,
// tile(s) = nt0 + GSTRIDE (s / 4) + s % 4: GSTRIDE = 4 is NT consecutive tiles (an MLP layer), 16 the same four hidden-column tiles of
// consecutive gates.  `act` points at the A column of k-group G0.  The weight stream is DEPTH k-groups deep; with an even DEPTH the next
// k-group's A fragments are read before the current one's MFMAs.  A fragment of k-step j: A[lane & 15][16 g + 4 j + (lane >> 4)]; B
// fragment: element j of the float4.
template <int NT, int KG, int DEPTH, int KTOT, int G0, int GSTRIDE>
__device__ __forceinline__ void contract(f32x4* acc, const float* __restrict__ wp, int nt0, const float* act, int stride, int lane) {
  static_assert(KG % DEPTH == 0 && G0 + KG <= KTOT, "k-groups: a multiple of the pipeline depth, inside the packed matrix");
  const f32x4* w4 = reinterpret_cast<const f32x4*>(wp) + ((size_t)nt0 * KTOT + G0) * 64 + lane;
  const float* arow = act + (lane & 15) * stride + (lane >> 4);
  f32x4 b[DEPTH][NT];
  float a[2][4];
#define ORR_STEP_TILE(s) ((GSTRIDE * ((s) / 4) + (s) % 4) * KTOT)
#pragma unroll
  for (int d = 0; d < DEPTH - 1; d++)
#pragma unroll
    for (int s = 0; s < NT; s++) b[d][s] = w4[(ORR_STEP_TILE(s) + d) * 64];
#pragma unroll
  for (int j = 0; j < 4; j++) a[0][j] = arow[4 * j];
#pragma unroll 1
  for (int g0 = 0; g0 < KG; g0 += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
      const int g = g0 + d;
      if (g + DEPTH - 1 < KG) {
#pragma unroll
        for (int s = 0; s < NT; s++) b[(d + DEPTH - 1) % DEPTH][s] = w4[(ORR_STEP_TILE(s) + g + DEPTH - 1) * 64];
      }
      if constexpr (DEPTH % 2 == 0) {
        if (g + 1 < KG) {
#pragma unroll
          for (int j = 0; j < 4; j++) a[(d + 1) & 1][j] = arow[16 * (g + 1) + 4 * j];
        }
      } else if (g > 0) {      // an odd depth: d does not tell the parity of g - the k-group's own fragments, read here
#pragma unroll
        for (int j = 0; j < 4; j++) a[d & 1][j] = arow[16 * g + 4 * j];
      }
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int s = 0; s < NT; s++) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[d & 1][j], b[d][s][j], acc[s], 0, 0, 0);
    }
  }
#undef ORR_STEP_TILE
}

// The K = 32 contraction over the frame for the wave's twelve tiles of Wx (acc[0..3]: the candidate's, acc[4..11]: r and u): both k-groups'
// weights in flight at once, the A words from the caller's registers.
__device__ __forceinline__ void contract_frame(f32x4* acc, const float* __restrict__ wx, int wave, const float (&x)[2][4], int lane) {
  constexpr int KG = kFrame / 16;
  const f32x4* w4 = reinterpret_cast<const f32x4*>(wx) + lane;
  f32x4 b[KG][12];
#pragma unroll
  for (int g = 0; g < KG; g++)
#pragma unroll
    for (int s = 0; s < 12; s++) {
      const int tile = s < 4 ? 32 + 4 * wave + s : 4 * wave + 16 * ((s - 4) / 4) + s % 4;
      b[g][s] = w4[(tile * KG + g) * 64];
    }
#pragma unroll
  for (int g = 0; g < KG; g++)
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int s = 0; s < 12; s++) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[g][j], b[g][s][j], acc[s], 0, 0, 0);
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

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

struct StepParams {
  orr_policy_net net;
  orr_gru_encoder enc;
  const float* obs;
  const uint8_t* start;
  const float* h0;
  const float* priv;
  const float* noise;
  float *action, *raw, *value, *mean, *hid, *latent;
  int n;
  float std, clip;
};

// layer 0 of one net for this wave (column tiles [8 wave, 8 wave + 8)): the 13 k-groups of its 208 x 512 matrix, ten from the observation's
// columns and three from `tail` (z or priv), twelve at depth 2 + the last one on its own (orr_policy.hip, ORR_POLICY_PRIV_SPLIT)
__device__ __forceinline__ void layer0(const float* __restrict__ w, const float* __restrict__ bias, const float* s_in, const float* tail, float* dst,
                                       int wave, int lane) {
  constexpr int KT = kNet / 16, KO = kObs / 16;
  f32x4 acc[8];
#pragma unroll
  for (int t = 0; t < 8; t++) acc[t] = f32x4{0, 0, 0, 0};
  contract<8, KO, 2, KT, 0, 4>(acc, w, 8 * wave, s_in, kInStride, lane);
  contract<8, 2, 2, KT, KO, 4>(acc, w, 8 * wave, tail, kInStride, lane);
  contract<8, 1, 1, KT, KO + 2, 4>(acc, w, 8 * wave, tail + 32, kInStride, lane);
  store_relu<8>(acc, bias, 8 * wave, dst, kH0Stride, lane);
}

__device__ __forceinline__ void layer1(const float* __restrict__ w, const float* __restrict__ bias, const float* src, float* dst, int wave, int lane) {
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = f32x4{0, 0, 0, 0};
  contract<4, kH0 / 16, 4, kH0 / 16, 0, 4>(acc, w, 4 * wave, src, kH0Stride, lane);
  store_relu<4>(acc, bias, 4 * wave, dst, kH1Stride, lane);
}

__global__ __launch_bounds__(256) void recurrent_step_kernel(StepParams P) {
  __shared__ float s_in[kRows * kInStride];
  __shared__ float s_h0[kRows * kH0Stride];      // first h' (stride kHStride)
  __shared__ float s_h1[kRows * kH1Stride];      // first h (stride kHStride)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * kRows;
  const int col = lane & 15, r0 = 4 * (lane >> 4);
  const bool critic = P.value != nullptr;        // kernel arguments: uniform over the workgroup, and every barrier is outside the tests on them
  const bool cpriv = critic && P.priv != nullptr;
  // ---- 1. the input tile and h' ----
  for (int i = tid; i < kRows * kObs; i += 256) {
    const int r = i / kObs, c = i - r * kObs;
    s_in[r * kInStride + c] = (row0 + r) < P.n ? P.obs[(size_t)(row0 + r) * kObs + c] : 0.0f;
  }
  {
    const int c = tid;                           // a thread owns one hidden column of the 16 rows
    static_assert(kHid == 256, "one hidden column per thread");
#pragma unroll 4
    for (int r = 0; r < kRows; r++) {
      const int robot = row0 + r;
      const bool live = robot < P.n && P.h0 && P.start && P.start[robot] == 0;
      s_h0[r * kHStride + c] = live ? P.h0[(size_t)robot * kHid + c] : 0.0f;
    }
  }
  if (cpriv) {
    for (int i = tid; i < kRows * kPriv; i += 256) {
      const int r = i / kPriv, c = i - r * kPriv;
      s_in[r * kInStride + kNet + c] = (row0 + r) < P.n ? P.priv[(size_t)(row0 + r) * kPriv + c] : 0.0f;
    }
  }
  // biases of this lane's hidden units
  float bxr[4], bxu[4], bxc[4], bhr[4], bhu[4], bhc[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int j = 64 * wave + 16 * i + col;
    bxr[i] = P.enc.bx[j]; bxu[i] = P.enc.bx[kHid + j]; bxc[i] = P.enc.bx[2 * kHid + j];
    bhr[i] = P.enc.bh[j]; bhu[i] = P.enc.bh[kHid + j]; bhc[i] = P.enc.bh[2 * kHid + j];
  }
  __syncthreads();
  // ---- 2. the gates ----
  {
    // the frame's A words of this lane: k = 16 g + 4 j + (lane >> 4) of obs[0:4] | obs[12:24] | obs[48:60] | 0 0 0 0
    float x[2][4];
#pragma unroll
    for (int g = 0; g < 2; g++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int k = 16 * g + 4 * j + (lane >> 4);
        const int src = k < 4 ? k : (k < 16 ? k + 8 : k + 32);
        x[g][j] = k < 28 ? s_in[col * kInStride + src] : 0.0f;
      }
    // accumulators: 0..3 the x-part of c, 4..7 r, 8..11 u, 12..15 q
    f32x4 acc[16];
#pragma unroll
    for (int s = 0; s < 16; s++) acc[s] = f32x4{0, 0, 0, 0};
    contract_frame(acc, P.enc.wx, wave, x, lane);
    contract<12, kHid / 16, 2, kHid / 16, 0, 16>(acc + 4, P.enc.wh, 4 * wave, s_h0, kHStride, lane);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int j = 64 * wave + 16 * i + col;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = r0 + r, robot = row0 + row;
        const float hp = s_h0[row * kHStride + j];
        const float rr = sigmoidf((acc[4 + i][r] + bxr[i]) + bhr[i]);
        const float uu = sigmoidf((acc[8 + i][r] + bxu[i]) + bhu[i]);
        const float q = acc[12 + i][r] + bhc[i];
        const float c = tanhf((acc[i][r] + bxc[i]) + rr * q);
        const float h = (1.0f - uu) * c + uu * hp;
        s_h1[row * kHStride + j] = h;
        if (robot < P.n) P.hid[(size_t)robot * kHid + j] = h;
      }
    }
  }
  __syncthreads();
  // ---- 3. z = h Wo + bo: one column tile on each of waves 0..2 ----
  if (wave < kPriv / 16) {
    f32x4 acc[1] = {f32x4{0, 0, 0, 0}};
    contract<1, kHid / 16, 4, kHid / 16, 0, 4>(acc, P.enc.wo, wave, s_h1, kHStride, lane);
    const int c = 16 * wave + col;
    const float b = P.enc.bo[c];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int robot = row0 + r0 + r;
      const float z = acc[0][r] + b;
      s_in[(r0 + r) * kInStride + kObs + c] = z;
      if (P.latent && robot < P.n) P.latent[(size_t)robot * kPriv + c] = z;
    }
  }
  __syncthreads();
  // ---- 4. layer 0: 208 -> 512 of each net ----
  layer0(P.net.w0_pi, P.net.b0_pi, s_in, s_in + kObs, s_h0, wave, lane);
  if (critic) layer0(P.net.w0_vf, P.net.b0_vf, s_in, s_in + (cpriv ? kNet : kObs), s_h0 + kH0, wave, lane);
  __syncthreads();
  // ---- 5. layer 1: 512 -> 256 ----
  layer1(P.net.w1_pi, P.net.b1_pi, s_h0, s_h1, wave, lane);
  if (critic) layer1(P.net.w1_vf, P.net.b1_vf, s_h0 + kH0, s_h1 + kH1, wave, lane);
  __syncthreads();
  // ---- 6. heads: wave 0 the actor (12 of 16 columns), wave 1 the critic (1 of 16 columns) ----
  if (wave >= 2) return;
  f32x4 acc[1] = {f32x4{0, 0, 0, 0}};
  if (wave == 0) {
    contract<1, kH1 / 16, 4, kH1 / 16, 0, 4>(acc, P.net.w2_pi, 0, s_h1, kH1Stride, lane);
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
  } else if (critic) {
    contract<1, kH1 / 16, 4, kH1 / 16, 0, 4>(acc, P.net.w2_vf, 0, s_h1 + kH1, kH1Stride, lane);
    if (col == 0) {
      const float b = P.net.b2_vf[0];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int robot = row0 + r0 + r;
        if (robot < P.n) P.value[robot] = acc[0][r] + b;
      }
    }
  }
}

inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

struct Range { const void* p; size_t bytes; };
inline bool overlap(const Range& a, const Range& b) {
  if (!a.p || !b.p) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
  return x < y + b.bytes && y < x + a.bytes;
}

}  // namespace

extern "C" {

int32_t orr_policy_forward_recurrent(const orr_policy_net* net, const orr_gru_encoder* enc, const float* obs, const uint8_t* start, const float* h0,
                                     const float* priv, int32_t n, const float* noise, float std, float clip, float* action, float* raw, float* value,
                                     float* mean, float* hid, float* latent, void* stream) {
  if (!net || !enc || !obs || !action || !hid || n < 1) return orr_fail(-1, "orr_policy_forward_recurrent: bad argument", hipSuccess);
  const float* const* p = reinterpret_cast<const float* const*>(net);
  for (int i = 0; i < 12; i++) {
    if (!p[i]) return orr_fail(-1, "orr_policy_forward_recurrent: orr_policy_net has a null pointer", hipSuccess);
    if (misaligned(p[i], i % 2 == 0 ? 15 : 3))       // packed weights are read 16 bytes per lane
      return orr_fail(-1, "orr_policy_forward_recurrent: packed weights must be 16-byte aligned, biases 4-byte aligned", hipSuccess);
  }
  const float* const* q = reinterpret_cast<const float* const*>(enc);
  for (int i = 0; i < 6; i++) {
    if (!q[i]) return orr_fail(-1, "orr_policy_forward_recurrent: orr_gru_encoder has a null pointer", hipSuccess);
    if (misaligned(q[i], i % 2 == 0 ? 15 : 3))
      return orr_fail(-1, "orr_policy_forward_recurrent: packed weights must be 16-byte aligned, biases 4-byte aligned", hipSuccess);
  }
  if (misaligned(hid, 15)) return orr_fail(-1, "orr_policy_forward_recurrent: hid must be 16-byte aligned", hipSuccess);
  for (const void* b : {(const void*)obs, (const void*)h0, (const void*)priv, (const void*)noise, (const void*)action, (const void*)raw,
                        (const void*)value, (const void*)mean, (const void*)latent})
    if (misaligned(b, 3)) return orr_fail(-1, "orr_policy_forward_recurrent: buffers must be 4-byte aligned", hipSuccess);
  const size_t rows = (size_t)n;
  const Range out[6] = {{hid, rows * kHid * 4}, {latent, rows * kPriv * 4}, {action, rows * kAct * 4}, {raw, rows * kAct * 4},
                        {mean, rows * kAct * 4}, {value, rows * 4}};
  const Range in[5] = {{h0, rows * kHid * 4}, {obs, rows * kObs * 4}, {start, rows}, {priv, rows * kPriv * 4}, {noise, rows * kAct * 4}};
  for (int i = 0; i < 6; i++) {
    for (int j = i + 1; j < 6; j++)
      if (overlap(out[i], out[j])) return orr_fail(-1, "orr_policy_forward_recurrent: outputs overlap", hipSuccess);
    for (int j = 0; j < 5; j++) {
      if (i == 0 && j == 0 && hid == h0) continue;   // the rollout's step in place: a workgroup reads its rows of h0 before it writes them
      if (overlap(out[i], in[j])) return orr_fail(-1, "orr_policy_forward_recurrent: an output overlaps an input (hid may BE h0)", hipSuccess);
    }
  }
  StepParams P;
  P.net = *net; P.enc = *enc; P.obs = obs; P.start = start; P.h0 = h0; P.priv = priv; P.noise = noise;
  P.action = action; P.raw = raw; P.value = value; P.mean = mean; P.hid = hid; P.latent = latent;
  P.n = n; P.std = std; P.clip = clip;
  hipLaunchKernelGGL(recurrent_step_kernel, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(256), 0, (hipStream_t)stream, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_policy_forward_recurrent: launch", e);
  return 0;
}

}  // extern "C"
