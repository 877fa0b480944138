// orr_recurrent.hip -- the recurrent history student: a GRU over the per-step sensor frame, forward and backward through time
// (include/openroborl_policy.h: orr_gru_forward; include/openroborl_learner.h: orr_gru_backward).
//
//   h'  = start_t ? 0 : h_{t-1}
//   r   = sigmoid(x_t Wx_r + h' Wh_r + bx_r + bh_r)        u = sigmoid(x_t Wx_u + h' Wh_u + bx_u + bh_u)
//   q   = h' Wh_c + bh_c                                    c = tanh(x_t Wx_c + bx_c + r q)
//   h_t = (1 - u) c + u h'                                  z_t = h_t Wo + bo
// with x_t the 32-word sensor frame of obs_t (obs[0:4] | obs[12:24] | obs[48:60] | 0 0 0 0, orr_history_push's frame).
//
// Mapping, both kernels: a workgroup of 256 threads (four waves, one per SIMD) owns 16 robots for ALL T steps; robots are the 16 rows of
// every matrix-core tile (v_mfma_f32_16x16x4_f32 = a k-ordered fmaf chain per element).  The 768 gate columns are split over the waves
// by HIDDEN column, not by gate: wave w owns hidden units 64 w .. 64 w + 63, i.e. column tiles 4 w .. 4 w + 3 of each of r, u and c.  In
// the accumulators' C layout (column = lane & 15, row = 4 (lane >> 4) + register) a lane therefore holds r, u, q and the x-part of c of
// the SAME (robot, hidden unit), and combines the gates without any exchange.  B operands are streamed from orr_policy_pack's fragment-major
// image, one 16-byte load per lane and tile for four k-steps, software-pipelined like orr_policy.hip's layer<>.
//
// Forward.  LDS: the hidden state as a 16 x 256 tile of stride 257 (odd: the 16 rows of an A fragment fall into distinct banks), twice, and
// the frame as a 16 x 32 tile of stride 33, twice.  Step t reads buffer t & 1 and writes h_t and x_{t+1} into the other one; ONE barrier
// per step separates the two, and nothing but the outputs goes through global memory between steps.  The tile holds h_{t-1} UNMASKED (the
// latent of step t - 1 is computed from it by waves 0..2 at the top of step t, K = 256 into one column tile each); the reset is applied
// where h' is consumed: an A fragment's row belongs to one robot (lane & 15), so a started robot's fragment is replaced by +0, which leaves
// the fmaf chain's value unchanged, and the combine reads h' = 0 for it.
// A pre-activation is ONE accumulator over k ascending - the 32 k of x, then the 256 k of h' - and then (acc + bx) + bh; the candidate keeps
// two, x Wx_c and h' Wh_c.  864 MFMAs per wave and step (+ 64 on three waves for the latent); the weight stream is 864 KB per workgroup and
// step out of L2.  expf / tanhf are the device library's (no fast-math forms).  T chained T = 1 calls run the same instructions on the same
// values as one call over T, hence its bits.  Rows at or beyond n read as zero, count as started and write nothing.
//
// Backward (truncated BPTT over the segment, t descending).  The carried dh lives in the owning lanes' accumulators (the same wave /
// hidden-column split, so the lane that needs u dh + ... is the lane that holds dh: it never goes through LDS); what goes through LDS is
// the A operand of the two contractions: g_latent_t as a 16 x 48 tile (stride 49) for dh += g_latent_t Wo^T (K = 48), and the step's g_h as
// a 16 x 768 tile (stride 769) for dh = u dh + g_h Wh^T (K = 768 into the wave's four column tiles), both double-buffered: one barrier per
// step again.  saved (r, u, c, q) and hprev are read at the accumulators' own coordinates.  Column sums of g_x and g_h (the bias gradients)
// are kept per lane over all steps and rows in a fixed order, folded over the four row groups with two shuffles at the end and left as one
// row per workgroup for orr_colsum_finish.  816 MFMAs per wave and step; the step t = 0 skips the K = 768 contraction (no gradient to h0).
// No atomics anywhere: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/openroborl_policy.h"
#include "../../include/openroborl_learner.h"

int orr_fail(int code, const char* msg, hipError_t e);  // orr_kernels.hip

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kObs = ORR_POLICY_OBS_DIM, kFrame = ORR_HISTORY_FRAME, kHid = ORR_GRU_HIDDEN, kGates = ORR_GRU_GATES, kLat = ORR_POLICY_PRIV_DIM;
constexpr int kRows = 16;                                  // robots per workgroup
constexpr int kHStride = kHid + 1, kXStride = kFrame + 1;   // odd strides: an A fragment's 16 rows in distinct LDS banks
constexpr int kGStride = kGates + 1, kLStride = kLat + 1;
static_assert(kHid == 256 && kGates == 3 * kHid && kFrame == 32 && kLat == 48, "four waves x four column tiles per gate; whole k-groups");
static_assert((2 * kRows * kGStride + 2 * kRows * kLStride) * sizeof(float) <= 160 * 1024, "static LDS beyond the 160 KB of a gfx950 CU");

// acc[s] += A(16 x 16 KGS, from LDS) * B(tile(s)) for NT column tiles of a packed (16 KGS) x . matrix: tile(s) = nt0 + GSTRIDE (s / 4) + s % 4
// (GSTRIDE = 16: the same four hidden-column tiles of consecutive gates).  The weight stream is DEPTH k-groups deep; with an even DEPTH the
// next k-group's A fragments are read before the current one's MFMAs.  zero_row: this lane's A row belongs to a robot that starts an
// episode - its fragments are +0.  A fragment of k-step j: A[lane & 15][16 g + 4 j + (lane >> 4)]; B fragment: element j of the float4.
template <int NT, int KGS, int DEPTH, int GSTRIDE>
__device__ __forceinline__ void contract(f32x4* acc, const float* __restrict__ wp, int nt0, const float* act, int stride, int lane, bool zero_row) {
  static_assert(KGS % DEPTH == 0, "k-groups must be a multiple of the pipeline depth");
  const f32x4* w4 = reinterpret_cast<const f32x4*>(wp) + (size_t)nt0 * KGS * 64 + lane;
  const float* arow = act + (lane & 15) * stride + (lane >> 4);
  f32x4 b[DEPTH][NT];
  float a[2][4];
#define ORR_GRU_TILE(s) ((GSTRIDE * ((s) / 4) + (s) % 4) * KGS)
#pragma unroll
  for (int d = 0; d < DEPTH - 1; d++)
#pragma unroll
    for (int s = 0; s < NT; s++) b[d][s] = w4[(ORR_GRU_TILE(s) + d) * 64];
#pragma unroll
  for (int j = 0; j < 4; j++) a[0][j] = zero_row ? 0.0f : arow[4 * j];
#pragma unroll 1
  for (int g0 = 0; g0 < KGS; g0 += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
      const int g = g0 + d;
      if (g + DEPTH - 1 < KGS) {
#pragma unroll
        for (int s = 0; s < NT; s++) b[(d + DEPTH - 1) % DEPTH][s] = w4[(ORR_GRU_TILE(s) + g + DEPTH - 1) * 64];
      }
      if constexpr (DEPTH % 2 == 0) {
        if (g + 1 < KGS) {
#pragma unroll
          for (int j = 0; j < 4; j++) a[(d + 1) & 1][j] = zero_row ? 0.0f : arow[16 * (g + 1) + 4 * j];
        }
      } else if (g > 0) {      // an odd depth: d does not tell the parity of g - the k-group's own fragments, read here
#pragma unroll
        for (int j = 0; j < 4; j++) a[d & 1][j] = zero_row ? 0.0f : arow[16 * g + 4 * j];
      }
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int s = 0; s < NT; s++) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[d & 1][j], b[d][s][j], acc[s], 0, 0, 0);
    }
  }
#undef ORR_GRU_TILE
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

struct FwdParams {
  orr_gru_encoder enc;
  const float* obs;
  const uint8_t* starts;
  const float* h0;
  int T, n;
  float *hid, *latent, *frames, *hprev, *saved;
};

// z_t = h_t Wo + bo from the unmasked tile of h_t: one column tile on each of waves 0..2
__device__ __forceinline__ void latent_out(const FwdParams& P, const float* h, int t, int row0, int wave, int lane) {
  if (wave >= kLat / 16) return;
  f32x4 acc[1] = {f32x4{0, 0, 0, 0}};
  contract<1, kHid / 16, 4, 0>(acc, P.enc.wo, wave, h, kHStride, lane, false);
  const int c = 16 * wave + (lane & 15), r0 = 4 * (lane >> 4);
  const float b = P.enc.bo[c];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int robot = row0 + r0 + r;
    if (robot < P.n) P.latent[((size_t)t * P.n + robot) * kLat + c] = acc[0][r] + b;
  }
}

__global__ __launch_bounds__(256) void gru_forward_kernel(FwdParams P) {
  __shared__ float s_h[2][kRows * kHStride];
  __shared__ float s_x[2][kRows * kXStride];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * kRows;
  const int col = lane & 15, r0 = 4 * (lane >> 4);
  const size_t n = (size_t)P.n;
  // the loader's share of a frame: row tid / 16, words 2 (tid % 16) and the next one; source column in obs, or -1 for the pad
  const int xrow = tid >> 4, xc = 2 * (tid & 15);
  const bool xlive = row0 + xrow < P.n;
  int xsrc[2];
#pragma unroll
  for (int e = 0; e < 2; e++) { const int c = xc + e; xsrc[e] = c < 4 ? c : (c < 16 ? c + 8 : (c < 28 ? c + 32 : -1)); }
  // biases of this lane's hidden units
  float bxr[4], bxu[4], bxc[4], bhr[4], bhu[4], bhc[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int j = 64 * wave + 16 * i + col;
    bxr[i] = P.enc.bx[j]; bxu[i] = P.enc.bx[kHid + j]; bxc[i] = P.enc.bx[2 * kHid + j];
    bhr[i] = P.enc.bh[j]; bhu[i] = P.enc.bh[kHid + j]; bhc[i] = P.enc.bh[2 * kHid + j];
  }
  // prologue: h0 (or zeros) and the frame of step 0 into buffer 0
  for (int i = tid; i < kRows * kHid; i += 256) {
    const int r = i / kHid, c = i - r * kHid;
    s_h[0][r * kHStride + c] = (P.h0 && row0 + r < P.n) ? P.h0[(size_t)(row0 + r) * kHid + c] : 0.0f;
  }
#pragma unroll
  for (int e = 0; e < 2; e++) {
    const float v = (xlive && xsrc[e] >= 0) ? P.obs[(size_t)(row0 + xrow) * kObs + xsrc[e]] : 0.0f;
    s_x[0][xrow * kXStride + xc + e] = v;
    if (P.frames && xlive) P.frames[(size_t)(row0 + xrow) * kFrame + xc + e] = v;
  }
  __syncthreads();
  for (int t = 0; t <= P.T; t++) {
    const int cur = t & 1, nxt = cur ^ 1;
    if (t > 0 && P.latent) latent_out(P, s_h[cur], t - 1, row0, wave, lane);
    if (t == P.T) break;
    // the next step's frame, in flight during this step's MFMAs
    float xn[2] = {0.0f, 0.0f};
    if (t + 1 < P.T && xlive) {
#pragma unroll
      for (int e = 0; e < 2; e++)
        if (xsrc[e] >= 0) xn[e] = P.obs[((size_t)(t + 1) * n + row0 + xrow) * kObs + xsrc[e]];
    }
    // who starts an episode at this step: the robot of this lane's A row, and the robots of its four C rows
    const bool start_a = (P.starts && row0 + col < P.n) ? P.starts[(size_t)t * n + row0 + col] != 0 : true;
    bool start_c[4];
#pragma unroll
    for (int r = 0; r < 4; r++) start_c[r] = (P.starts && row0 + r0 + r < P.n) ? P.starts[(size_t)t * n + row0 + r0 + r] != 0 : true;
    // accumulators: 0..3 the x-part of c, 4..7 r, 8..11 u, 12..15 q
    f32x4 acc[16];
#pragma unroll
    for (int s = 0; s < 16; s++) acc[s] = f32x4{0, 0, 0, 0};
    contract<4, kFrame / 16, 2, 0>(acc, P.enc.wx, 32 + 4 * wave, s_x[cur], kXStride, lane, false);
    contract<8, kFrame / 16, 2, 16>(acc + 4, P.enc.wx, 4 * wave, s_x[cur], kXStride, lane, false);
    contract<12, kHid / 16, 2, 16>(acc + 4, P.enc.wh, 4 * wave, s_h[cur], kHStride, lane, start_a);
    // the gates of this lane's 16 (robot, hidden unit) pairs
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int j = 64 * wave + 16 * i + col;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = r0 + r, robot = row0 + row;
        const float hp = start_c[r] ? 0.0f : s_h[cur][row * kHStride + j];
        const float rr = sigmoidf((acc[4 + i][r] + bxr[i]) + bhr[i]);
        const float uu = sigmoidf((acc[8 + i][r] + bxu[i]) + bhu[i]);
        const float q = acc[12 + i][r] + bhc[i];
        const float c = tanhf((acc[i][r] + bxc[i]) + rr * q);
        const float h = (1.0f - uu) * c + uu * hp;
        s_h[nxt][row * kHStride + j] = h;
        if (robot < P.n) {
          const size_t o = (size_t)t * n + robot;
          P.hid[o * kHid + j] = h;
          if (P.hprev) P.hprev[o * kHid + j] = hp;
          if (P.saved) {
            float* sv = P.saved + o * (4 * kHid) + j;
            sv[0] = rr; sv[kHid] = uu; sv[2 * kHid] = c; sv[3 * kHid] = q;
          }
        }
      }
    }
    if (t + 1 < P.T) {
#pragma unroll
      for (int e = 0; e < 2; e++) {
        s_x[nxt][xrow * kXStride + xc + e] = xn[e];
        if (P.frames && xlive) P.frames[((size_t)(t + 1) * n + row0 + xrow) * kFrame + xc + e] = xn[e];
      }
    }
    __syncthreads();
  }
}

struct BwdParams {
  orr_gru_transposed enc;
  const float *g_latent, *saved, *hprev;
  const uint8_t* starts;
  int T, n;
  float *g_x, *g_h, *partials;
};

__global__ __launch_bounds__(256) void gru_backward_kernel(BwdParams P) {
  __shared__ float s_g[2][kRows * kGStride];
  __shared__ float s_l[2][kRows * kLStride];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * kRows;
  const int col = lane & 15, r0 = 4 * (lane >> 4);
  const size_t n = (size_t)P.n;
  constexpr int kLoads = kRows * kLat / 256;      // the loader's share of a g_latent tile: three words
  static_assert(kLoads * 256 == kRows * kLat, "whole words per thread");
  {
    const int t = P.T - 1;
#pragma unroll
    for (int e = 0; e < kLoads; e++) {
      const int i = tid + 256 * e, r = i / kLat, c = i - r * kLat;
      s_l[t & 1][r * kLStride + c] = row0 + r < P.n ? P.g_latent[((size_t)t * n + row0 + r) * kLat + c] : 0.0f;
    }
  }
  __syncthreads();
  f32x4 dh[4];                                    // the carried gradient at this lane's 16 (robot, hidden unit) pairs
  float sr[4], su[4], sc[4], sq[4];               // column sums of dr_pre, du_pre, dc_pre and r dc_pre over this lane's rows and all steps
#pragma unroll
  for (int i = 0; i < 4; i++) { dh[i] = f32x4{0, 0, 0, 0}; sr[i] = su[i] = sc[i] = sq[i] = 0.0f; }
  for (int t = P.T - 1; t >= 0; t--) {
    const int cur = t & 1, nxt = cur ^ 1;
    float gl[kLoads];                             // the tile of step t - 1, in flight during this step
#pragma unroll
    for (int e = 0; e < kLoads; e++) {
      const int i = tid + 256 * e, r = i / kLat, c = i - r * kLat;
      gl[e] = (t > 0 && row0 + r < P.n) ? P.g_latent[((size_t)(t - 1) * n + row0 + r) * kLat + c] : 0.0f;
    }
    float vr[4][4], vu[4][4], vc[4][4], vq[4][4], vh[4][4];
    bool start_c[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int robot = row0 + r0 + r;
      const bool live = robot < P.n;
      start_c[r] = (P.starts && live) ? P.starts[(size_t)t * n + robot] != 0 : true;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int j = 64 * wave + 16 * i + col;
        const size_t o = (size_t)t * n + (live ? robot : 0);
        const float* sv = P.saved + o * (4 * kHid) + j;
        vr[i][r] = live ? sv[0] : 0.0f; vu[i][r] = live ? sv[kHid] : 0.0f; vc[i][r] = live ? sv[2 * kHid] : 0.0f;
        vq[i][r] = live ? sv[3 * kHid] : 0.0f; vh[i][r] = live ? P.hprev[o * kHid + j] : 0.0f;
      }
    }
    contract<4, kLat / 16, 3, 0>(dh, P.enc.wot, 4 * wave, s_l[cur], kLStride, lane, false);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int j = 64 * wave + 16 * i + col;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = r0 + r, robot = row0 + row;
        const float d = dh[i][r], rr = vr[i][r], uu = vu[i][r], c = vc[i][r], q = vq[i][r];
        const float du = d * (vh[i][r] - c), dc = d * (1.0f - uu);
        const float dcp = dc * (1.0f - c * c), dup = du * uu * (1.0f - uu);
        const float drp = dcp * q * rr * (1.0f - rr), gc = rr * dcp;
        float* g = s_g[cur] + row * kGStride + j;
        g[0] = drp; g[kHid] = dup; g[2 * kHid] = gc;
        if (robot < P.n) {
          const size_t o = ((size_t)t * n + robot) * kGates + j;
          P.g_x[o] = drp; P.g_x[o + kHid] = dup; P.g_x[o + 2 * kHid] = dcp;
          P.g_h[o] = drp; P.g_h[o + kHid] = dup; P.g_h[o + 2 * kHid] = gc;
        }
        sr[i] += drp; su[i] += dup; sc[i] += dcp; sq[i] += gc;
        dh[i][r] = uu * d;
      }
    }
    if (t == 0) break;                            // no gradient with respect to h0
#pragma unroll
    for (int e = 0; e < kLoads; e++) {
      const int i = tid + 256 * e, r = i / kLat, c = i - r * kLat;
      s_l[nxt][r * kLStride + c] = gl[e];
    }
    __syncthreads();
    contract<4, kGates / 16, 4, 0>(dh, P.enc.wht, 4 * wave, s_g[cur], kGStride, lane, false);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        if (start_c[r]) dh[i][r] = 0.0f;          // h' of a started robot was 0, not h_{t-1}: nothing flows into the earlier step
  }
  // the four row groups of a column, in a fixed order; one row of partials per workgroup: [768] of g_x, and behind all rows [768] of g_h
  float* px = P.partials + (size_t)blockIdx.x * kGates;
  float* ph = P.partials + ((size_t)gridDim.x + blockIdx.x) * kGates;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int j = 64 * wave + 16 * i + col;
    float v[4] = {sr[i], su[i], sc[i], sq[i]};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      v[k] += __shfl_xor(v[k], 16, 64);
      v[k] += __shfl_xor(v[k], 32, 64);
    }
    if (lane < 16) {
      px[j] = v[0]; px[kHid + j] = v[1]; px[2 * kHid + j] = v[2];
      ph[j] = v[0]; ph[kHid + j] = v[1]; ph[2 * kHid + j] = v[3];
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
template <int N>
inline bool any_overlap(const Range (&r)[N]) {
  for (int i = 0; i < N; i++)
    for (int j = i + 1; j < N; j++)
      if (overlap(r[i], r[j])) return true;
  return false;
}

}  // namespace

extern "C" {

int32_t orr_gru_forward(const orr_gru_encoder* enc, const float* obs, const uint8_t* starts, const float* h0, int32_t t, int32_t n, float* hid,
                        float* latent, float* frames, float* hprev, float* saved, void* stream) {
  if (!enc || !obs || !hid || t < 1 || n < 1) return orr_fail(-1, "orr_gru_forward: bad argument", hipSuccess);
  if (!starts && t != 1) return orr_fail(-1, "orr_gru_forward: starts == NULL (everybody starts) goes with T = 1 only", hipSuccess);
  const float* const* p = reinterpret_cast<const float* const*>(enc);
  for (int i = 0; i < 6; i++) {
    if (!p[i]) return orr_fail(-1, "orr_gru_forward: orr_gru_encoder has a null pointer", hipSuccess);
    if (misaligned(p[i], i % 2 == 0 ? 15 : 3))     // packed weights are read 16 bytes per lane
      return orr_fail(-1, "orr_gru_forward: packed weights must be 16-byte aligned, biases 4-byte aligned", hipSuccess);
  }
  if (misaligned(hid, 15) || misaligned(saved, 15)) return orr_fail(-1, "orr_gru_forward: hid and saved must be 16-byte aligned", hipSuccess);
  for (const void* q : {(const void*)obs, (const void*)h0, (const void*)latent, (const void*)frames, (const void*)hprev})
    if (misaligned(q, 3)) return orr_fail(-1, "orr_gru_forward: buffers must be 4-byte aligned", hipSuccess);
  const size_t rows = (size_t)t * (size_t)n;
  const Range out[5] = {{hid, rows * kHid * 4}, {latent, rows * kLat * 4}, {frames, rows * kFrame * 4}, {hprev, rows * kHid * 4},
                        {saved, rows * 4 * kHid * 4}};
  if (any_overlap(out)) return orr_fail(-1, "orr_gru_forward: outputs overlap", hipSuccess);
  const Range in[3] = {{obs, rows * kObs * 4}, {starts, rows}, {h0, (size_t)n * kHid * 4}};
  for (int i = 0; i < 5; i++)
    for (int j = 0; j < 3; j++) {
      if (i == 0 && j == 2 && t == 1 && hid == h0) continue;      // the rollout's step in place: every read of a row precedes its writes
      if (overlap(out[i], in[j])) return orr_fail(-1, "orr_gru_forward: an output overlaps an input (hid may BE h0 with T = 1 only)", hipSuccess);
    }
  FwdParams P;
  P.enc = *enc; P.obs = obs; P.starts = starts; P.h0 = h0; P.T = t; P.n = n;
  P.hid = hid; P.latent = latent; P.frames = frames; P.hprev = hprev; P.saved = saved;
  hipLaunchKernelGGL(gru_forward_kernel, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(256), 0, (hipStream_t)stream, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_gru_forward: launch", e);
  return 0;
}

int32_t orr_gru_backward(const orr_gru_transposed* enc, const float* g_latent, const float* saved, const float* hprev, const uint8_t* starts,
                         int32_t t, int32_t n, float* g_x, float* g_h, float* partials, void* stream) {
  if (!enc || !enc->wht || !enc->wot || !g_latent || !saved || !hprev || !starts || !g_x || !g_h || !partials || t < 1 || n < 1)
    return orr_fail(-1, "orr_gru_backward: bad argument", hipSuccess);
  if (misaligned(enc->wht, 15) || misaligned(enc->wot, 15) || misaligned(saved, 15) || misaligned(g_x, 15) || misaligned(g_h, 15))
    return orr_fail(-1, "orr_gru_backward: packed weights, saved, g_x and g_h must be 16-byte aligned", hipSuccess);
  for (const void* q : {(const void*)g_latent, (const void*)hprev, (const void*)partials})
    if (misaligned(q, 3)) return orr_fail(-1, "orr_gru_backward: buffers must be 4-byte aligned", hipSuccess);
  const size_t rows = (size_t)t * (size_t)n;
  const Range out[3] = {{g_x, rows * kGates * 4}, {g_h, rows * kGates * 4}, {partials, (size_t)ORR_GRU_BACKWARD_PARTIAL_FLOATS(n) * 4}};
  if (any_overlap(out)) return orr_fail(-1, "orr_gru_backward: outputs overlap", hipSuccess);
  const Range in[4] = {{g_latent, rows * kLat * 4}, {saved, rows * 4 * kHid * 4}, {hprev, rows * kHid * 4}, {starts, rows}};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++)
      if (overlap(out[i], in[j])) return orr_fail(-1, "orr_gru_backward: an output overlaps an input", hipSuccess);
  BwdParams P;
  P.enc = *enc; P.g_latent = g_latent; P.saved = saved; P.hprev = hprev; P.starts = starts; P.T = t; P.n = n;
  P.g_x = g_x; P.g_h = g_h; P.partials = partials;
  hipLaunchKernelGGL(gru_backward_kernel, dim3((unsigned)ORR_GRU_BACKWARD_ROWS(n)), dim3(256), 0, (hipStream_t)stream, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return orr_fail(-2, "orr_gru_backward: launch", e);
  return 0;
}

}  // extern "C"
