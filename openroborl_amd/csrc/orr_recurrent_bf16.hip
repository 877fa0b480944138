// orr_recurrent_bf16.hip -- the recurrent history student's GRU on the bf16 matrix cores: orr_gru_pack_bf16, orr_gru_forward_bf16
// (include/openroborl_policy.h) and orr_gru_backward_bf16 (include/openroborl_learner.h); host side: policy_hip.GruEncoder(bf16=True),
// learner_hip.FusedDistillRecurrent(bf16_gemm=True).  A translation unit of its own: orr_recurrent.hip and every other kernel compile exactly
// as they did.  The recurrence, the gate order, the outputs and the partials are orr_recurrent.hip's; what differs is the contractions' data
// type, in the sense of orr_learner_bf16.hip: every buffer in memory is float32, the operands of v_mfma_f32_16x16x32_bf16 are rounded to bf16
// (nearest even) on their way to the matrix cores, the accumulators and everything after them are float32.
//
// Where the rounding happens.  The MLP kernels read each weight once per launch and round it in the stage.  The GRU reads each weight T times
// per launch from every workgroup, so the weights are rounded ONCE, by orr_gru_pack_bf16, into a packed, derived image like orr_policy_pack's
// (re-made when the weights move): for column tile nt and k-step ks (32 k) lane l owns the eight elements W[32 ks + 8 (l >> 4) + e][16 nt +
// (l & 15)], one 16-byte load per lane, 1 KB per tile and k-step, coalesced.  With `transpose` the image of W^T is written straight from W.
// Activations (the frame x_t, the masked state h', h_t for the latent; g_latent_t and the step's g_h in the backward) are rounded as they are
// stored to LDS, once per element; the f32 values stay in the owning lanes' registers and are what goes to memory and into the combine.
//
// Mapping, both kernels: orr_recurrent.hip's.  A workgroup of 256 threads (four waves) owns 16 robots for ALL T steps, robots are the 16 rows
// of every tile, wave w owns hidden units 64 w .. 64 w + 63 of each gate, so that in the C layout (column = lane & 15, row = 4 (lane >> 4) +
// register) a lane holds r, u, q and the x-part of c of the SAME (robot, hidden unit) and combines the gates without an exchange.
//
// Forward.  108 MFMAs per wave and step (12 for x, 96 for h'; + 8 on three waves for the latent) instead of 864: the step is no longer bound
// by the matrix cores but by the weight stream's latency, the LDS round trip of h and the transcendental gates.  Hence:
//   * Wx (48 KB) and Wo (24 KB) are copied to LDS once per launch and read from there as B fragments (ds_read_b128, a fragment is 1 KB of
//     consecutive addresses: no bank conflict).  Wh, 384 KB per workgroup and step out of L2, is the only per-step stream.
//   * The Wh stream is a ring of FOUR k-steps x 12 tiles in registers (192 VGPRs, 36 KB per wave in flight).  8 k-steps per step is a whole
//     number of ring turns, so the slots are compile-time registers and the ring runs ACROSS steps: the first three k-steps of step t + 1 are
//     requested during the last three of step t and are in flight behind the gates, the stores and the barrier.
//   * The hidden state goes into LDS already rounded, a 16 x 256 bf16 tile of stride 256 + 8 (132 words = 4 mod 64: the sixteen 16-byte
//     reads of a quarter wave cover the 64 banks once), double-buffered, ONE barrier per step; a k-step's A fragment is one ds_read_b128.  The
//     frame tile is 16 x 32 of stride 32 + 8 (20 words: the same property).  The tile holds h_{t-1} unmasked (the latent reads it); a started
//     robot's A fragment is replaced by +0.
//   * The lane that writes h[row][j] is the lane that needs h'[row][j] in the next combine: the f32 h' stays in 16 registers and is never
//     read back from LDS.  hprev[t] is therefore bit for bit starts[t] ? 0 : hid[t - 1], and the A operand of step t is RNE_bf16(hprev[t]).
// A pre-activation is one accumulator over x then h', then (acc + bx) + bh; expf / tanhf are the device library's.  T chained T = 1 calls run
// the same instructions on the same values as one call over T, hence its bits.  Rows at or beyond n read as zero, count as started and
// write nothing.  No atomics, no scratch.
//
// Backward (t descending).  dh is carried in the owning lanes' accumulators as in the f32 kernel.  Through LDS go the rounded A operands:
// g_latent_t as a 16 x 64 bf16 tile (48 columns + 16 zeros, stride 72) and the step's g_h as a 16 x 768 tile of stride 776 (388 words = 4 mod
// 64), both double-buffered: one barrier per step.  Wo^T's share of a wave (4 tiles x 2 k-steps, rows 48..63 of the image are zero) stays
// in 32 VGPRs for the whole launch; Wh^T (384 KB per workgroup and step) streams through a ring of EIGHT k-steps x 4 tiles (128 VGPRs, 32 KB
// per wave in flight; 24 k-steps = three turns, so the ring runs across steps here too).  saved and hprev of step t - 1 (80 words per lane,
// out of HBM) are requested behind the barrier of step t and arrive under its contraction.  104 MFMAs per wave and step instead of 816.
// Column sums as in the f32 kernel: per lane in a fixed order, two shuffles, one row of partials per workgroup for orr_colsum_finish.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950, the unit's flags in _lib.py: -O3 without the packed-fp32 operations; with them
// the forward is 254 + 154 and the backward 256 + 200), no scratch:
//   gru_forward_bf16_kernel    255 VGPRs + 158 AGPRs, LDS 93184 bytes, 1 wave per SIMD
//   gru_backward_bf16_kernel   256 VGPRs + 251 AGPRs, LDS 54272 bytes, 1 wave per SIMD
// Both kernels spend their registers on the depth of the stream and run one workgroup per CU.  The backward's LDS (54 KB, a quarter of the
// f32 kernel's g_h tile) would allow two, its registers do not; at every shape the project runs (4096 robots in the rollout, 512 .. 4096 in
// a minibatch) there are at most 256 workgroups for 256 CUs, so a second resident workgroup would stay empty: not built, no number.
// Measured (profiles/gru_bf16.txt, MI355X, 4096 robots, against the f32 kernels in the same process): T = 1 forward 26.7 -> 17.0 us, T = 32
// forward 717 -> 286 us (22.4 -> 8.9 us per step), with the training outputs 813 -> 369 us, T = 32 backward 746 -> 440 us (its step still
// reads saved / hprev and writes g_x / g_h in f32, 176 words per lane).  Ring depths: with both rings halved (forward 2, backward 4 k-steps)
// the T = 32 forward takes 292 instead of 285 us and the backward 448 instead of 441 us - the depth buys 2.5 % and 1.6 %, it is not what
// bounds the step.
// Tried and dropped:
//   * fragment addresses left to the compiler: it keeps one 64-bit VECTOR address per fragment alive over the loop over the steps (96 pairs)
//     and spills - 292 bytes of scratch per lane in the forward, 696 in the backward (the compiler's report; never run: the unit builds
//     without scratch).  Hence frag_base(): a fragment's address is uniform, pinned to an SGPR pair at its use, and the load is scalar
//     base + 16 lane.
//   * per-element `robot < n ? load : 0` and per-element guarded stores: a branch each, 100 basic blocks per step (the compiler's report;
//     never run).  A row's loads are now unconditional from a clamped row and selected, its stores sit behind one branch.
//   * Wx resident in 48 VGPRs: it fits only beside a ring of two k-steps (12 KB per wave in flight); in LDS it costs no register, and the
//     ring is four deep.  The variant itself was not built; the two-deep Wh ring it would have had is the 292 us above.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/openroborl_policy.h"
#include "../../include/openroborl_learner.h"

int orr_fail(int code, const char* msg, hipError_t e);  // orr_kernels.hip

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kObs = ORR_POLICY_OBS_DIM, kFrame = ORR_HISTORY_FRAME, kHid = ORR_GRU_HIDDEN, kGates = ORR_GRU_GATES, kLat = ORR_POLICY_PRIV_DIM;
constexpr int kRows = 16;                                   // robots per workgroup
constexpr int kFrag = 512;                                  // bf16 elements of one (tile, k-step) fragment of an image: 64 lanes x 8
constexpr int kHS = kHid + 8, kXS = kFrame + 8;             // LDS row strides in bf16: 4 words mod 64 resp. 20 words, see above
constexpr int kGS = kGates + 8, kLK = 64, kLS = kLK + 8;    // backward: g_h tile; g_latent tile of 48 columns + 16 zeros
constexpr int kHK = kHid / 32, kGK = kGates / 32;           // k-steps of the h' contraction (8) and of g_h Wh^T (24)
constexpr int kFwdDepth = 4, kBwdDepth = 8;                 // k-steps in the weight rings
static_assert(kHid == 256 && kGates == 3 * kHid && kFrame == 32 && kLat == 48, "four waves x four column tiles per gate; whole k-steps");
static_assert(kHK % kFwdDepth == 0 && kGK % kBwdDepth == 0, "whole ring turns per step: the slots are compile-time registers");

__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ bf16x8 zero8() {
  const __bf16 z = (__bf16)0.0f;
  return bf16x8{z, z, z, z, z, z, z, z};
}
// A row's base address, opaque to the optimiser: the accesses of a row are then this register pair + a constant offset
// (every offset within a row fits the instruction's immediate), not an address of their own each.
template <typename T>
__device__ __forceinline__ T* row_base(T* p) {
  asm("" : "+v"(p));
  return p;
}
// A fragment's uniform address, pinned to an SGPR pair where it is used: the load is then scalar base + the lane's 32-bit offset.  (Left
// to itself the compiler hoists a VECTOR address per fragment out of the loop over the steps - 96 register pairs - and spills.)
__device__ __forceinline__ const char* frag_base(const char* p) {
  asm volatile("" : "+s"(p));
  return p;
}
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- orr_gru_pack_bf16 ----------------------------------------------------------------------------------------------------------------------
// one thread per (tile, k-step, lane): eight elements, each rounded once, one 16-byte store
__global__ __launch_bounds__(256) void pack_bf16_kernel(const float* __restrict__ w, int k, int n, int transpose, __bf16* __restrict__ out, int ksteps,
                                                        long long total) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int l = (int)(g & 63), ks = (int)((g >> 6) % ksteps), nt = (int)((g >> 6) / ksteps);
  const int K = transpose ? n : k, N = transpose ? k : n;         // the image's matrix: w, or w^T
  const int c = 16 * nt + (l & 15), k0 = 32 * ks + 8 * (l >> 4);
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const int kk = k0 + e;
    const float x = (kk < K && c < N) ? (transpose ? w[(size_t)c * n + kk] : w[(size_t)kk * n + c]) : 0.0f;
    v[e] = (__bf16)x;
  }
  reinterpret_cast<bf16x8*>(out)[g] = v;
}

// ---- forward --------------------------------------------------------------------------------------------------------------------------------
struct FwdParams {
  const __bf16 *wx, *wh, *wo;
  const float *bx, *bh, *bo;
  const float* obs;
  const uint8_t* starts;
  const float* h0;
  int T, n;
  float *hid, *latent, *frames, *hprev, *saved;
};

// the wave's twelve Wh fragments of k-step ks: hidden-column tiles 4 wave + s % 4 of gate s / 4.  wh: the image + the wave's tile, a UNIFORM
// address, lane16 = 16 lane: a load is scalar base + one VGPR of offset (a vector address per fragment would be 192 VGPRs of addresses)
__device__ __forceinline__ void fetch_wh(bf16x8 (&b)[12], const char* __restrict__ wh, uint32_t lane16, int ks) {
#pragma unroll
  for (int s = 0; s < 12; s++) b[s] = *reinterpret_cast<const bf16x8*>(frag_base(wh + ((16 * (s / 4) + s % 4) * kHK + ks) * (kFrag * 2)) + lane16);
}

// z_t = h_t Wo + bo from the unmasked rounded tile of h_t: one column tile on each of waves 0..2, Wo's fragments from LDS
__device__ __forceinline__ void latent_out(const FwdParams& P, const __bf16* h, const __bf16* s_wo, int t, int row0, int wave, int lane) {
  if (wave >= kLat / 16) return;
  f32x4 acc = f32x4{0, 0, 0, 0};
  const __bf16* arow = h + (lane & 15) * kHS + 8 * (lane >> 4);
#pragma unroll
  for (int ks = 0; ks < kHK; ks++)
    acc = mfma(*reinterpret_cast<const bf16x8*>(arow + 32 * ks), *reinterpret_cast<const bf16x8*>(s_wo + (wave * kHK + ks) * kFrag + 8 * lane), acc);
  const int c = 16 * wave + (lane & 15), r0 = 4 * (lane >> 4);
  const float b = P.bo[c];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int robot = row0 + r0 + r;
    if (robot < P.n) P.latent[((size_t)t * P.n + robot) * kLat + c] = acc[r] + b;
  }
}

__global__ __launch_bounds__(256) void gru_forward_bf16_kernel(FwdParams P) {
  __shared__ __attribute__((aligned(16))) __bf16 s_wx[(kGates / 16) * kFrag];      // 48 KB: Wx's image, 48 tiles x one k-step
  __shared__ __attribute__((aligned(16))) __bf16 s_wo[(kLat / 16) * kHK * kFrag];  // 24 KB: Wo's image, 3 tiles x 8 k-steps
  __shared__ __attribute__((aligned(16))) __bf16 s_h[2][kRows * kHS];
  __shared__ __attribute__((aligned(16))) __bf16 s_x[2][kRows * kXS];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;      // wave: uniform, in an SGPR
  const int row0 = blockIdx.x * kRows;
  const int col = lane & 15, r0 = 4 * (lane >> 4);
  const size_t n = (size_t)P.n;
  // the Wh ring: the first three k-steps of step 0 are requested before anything else
  const char* wh = reinterpret_cast<const char*>(P.wh) + (size_t)(4 * wave) * kHK * (kFrag * 2);
  const uint32_t lane16 = 16 * lane;
  bf16x8 ring[kFwdDepth][12];
#pragma unroll
  for (int d = 0; d < kFwdDepth - 1; d++) fetch_wh(ring[d], wh, lane16, d);
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
    bxr[i] = P.bx[j]; bxu[i] = P.bx[kHid + j]; bxc[i] = P.bx[2 * kHid + j];
    bhr[i] = P.bh[j]; bhu[i] = P.bh[kHid + j]; bhc[i] = P.bh[2 * kHid + j];
  }
  // prologue: the two resident images, 16 bytes per thread and trip
  for (int i = tid; i < (kGates / 16) * kFrag / 8; i += 256) reinterpret_cast<bf16x8*>(s_wx)[i] = reinterpret_cast<const bf16x8*>(P.wx)[i];
  for (int i = tid; i < (kLat / 16) * kHK * kFrag / 8; i += 256) reinterpret_cast<bf16x8*>(s_wo)[i] = reinterpret_cast<const bf16x8*>(P.wo)[i];
  // h0 (or zeros) at this lane's own 16 (robot, hidden unit) pairs: f32 into registers, rounded into buffer 0
  float hreg[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int j = 64 * wave + 16 * i + col;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = r0 + r;
      const float v = (P.h0 && row0 + row < P.n) ? P.h0[(size_t)(row0 + row) * kHid + j] : 0.0f;
      hreg[i][r] = v;
      s_h[0][row * kHS + j] = (__bf16)v;
    }
  }
  {  // the frame of step 0
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
      v[e] = (xlive && xsrc[e] >= 0) ? P.obs[(size_t)(row0 + xrow) * kObs + xsrc[e]] : 0.0f;
      if (P.frames && xlive) P.frames[(size_t)(row0 + xrow) * kFrame + xc + e] = v[e];
    }
    *reinterpret_cast<bf16x2*>(&s_x[0][xrow * kXS + xc]) = bf16x2{(__bf16)v[0], (__bf16)v[1]};
  }
  __syncthreads();
  for (int t = 0; t <= P.T; t++) {
    const int cur = t & 1, nxt = cur ^ 1;
    if (t > 0 && P.latent) latent_out(P, s_h[cur], s_wo, t - 1, row0, wave, lane);
    if (t == P.T) break;
    const bool more = t + 1 < P.T;
    // the next step's frame, in flight during this step's MFMAs
    float xn[2] = {0.0f, 0.0f};
    if (more && xlive) {
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
    {
      const bf16x8 ax = *reinterpret_cast<const bf16x8*>(&s_x[cur][col * kXS + 8 * (lane >> 4)]);
      const __bf16* wxl = s_wx + (4 * wave) * kFrag + 8 * lane;
#pragma unroll
      for (int s = 0; s < 12; s++) {    // s / 4: gate r, u, c -> accumulators 4.., 8.., 0..
        const int a = (4 + s) % 12;
        acc[a] = mfma(ax, *reinterpret_cast<const bf16x8*>(wxl + (16 * (s / 4) + s % 4) * kFrag), acc[a]);
      }
    }
    const __bf16* arow = s_h[cur] + col * kHS + 8 * (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < kHK; ks++) {
      if (ks + kFwdDepth - 1 < kHK || more) fetch_wh(ring[(ks + kFwdDepth - 1) % kFwdDepth], wh, lane16, (ks + kFwdDepth - 1) % kHK);
      const bf16x8 ah = start_a ? zero8() : *reinterpret_cast<const bf16x8*>(arow + 32 * ks);
#pragma unroll
      for (int s = 0; s < 12; s++) acc[4 + s] = mfma(ah, ring[ks % kFwdDepth][s], acc[4 + s]);
      __builtin_amdgcn_sched_barrier(0);          // keep the ring as written: no request moves up across a k-step
    }
    // the gates of this lane's 16 (robot, hidden unit) pairs, a row (robot) at a time
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = r0 + r, robot = row0 + row;
      const bool live = robot < P.n;
      const size_t o = (size_t)t * n + (live ? robot : 0);
      const int j0 = 64 * wave + col;
      float* hid_r = row_base(P.hid + o * kHid + j0);
      float* hprev_r = P.hprev ? row_base(P.hprev + o * kHid + j0) : nullptr;
      float* saved_r = P.saved ? row_base(P.saved + o * (4 * kHid) + j0) : nullptr;
      float vh[4], vp[4], vr[4], vu[4], vc[4], vq[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float hp = start_c[r] ? 0.0f : hreg[i][r];
        const float rr = sigmoidf((acc[4 + i][r] + bxr[i]) + bhr[i]);
        const float uu = sigmoidf((acc[8 + i][r] + bxu[i]) + bhu[i]);
        const float q = acc[12 + i][r] + bhc[i];
        const float c = tanhf((acc[i][r] + bxc[i]) + rr * q);
        const float h = (1.0f - uu) * c + uu * hp;
        hreg[i][r] = h;
        s_h[nxt][row * kHS + j0 + 16 * i] = (__bf16)h;
        vh[i] = h; vp[i] = hp; vr[i] = rr; vu[i] = uu; vc[i] = c; vq[i] = q;
      }
      if (live) {                                 // the row's stores behind one branch
#pragma unroll
        for (int i = 0; i < 4; i++) hid_r[16 * i] = vh[i];
        if (hprev_r) {
#pragma unroll
          for (int i = 0; i < 4; i++) hprev_r[16 * i] = vp[i];
        }
        if (saved_r) {
#pragma unroll
          for (int i = 0; i < 4; i++) {
            float* sv = saved_r + 16 * i;
            sv[0] = vr[i]; sv[kHid] = vu[i]; sv[2 * kHid] = vc[i]; sv[3 * kHid] = vq[i];
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);          // four pairs at a time: sixteen interleaved expf / tanhf would take the ring's registers
    }
    if (more) {
      *reinterpret_cast<bf16x2*>(&s_x[nxt][xrow * kXS + xc]) = bf16x2{(__bf16)xn[0], (__bf16)xn[1]};
      if (P.frames && xlive) {
#pragma unroll
        for (int e = 0; e < 2; e++) P.frames[((size_t)(t + 1) * n + row0 + xrow) * kFrame + xc + e] = xn[e];
      }
    }
    __syncthreads();
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------------------
struct BwdParams {
  const __bf16 *wht, *wot;
  const float *g_latent, *saved, *hprev;
  const uint8_t* starts;
  int T, n;
  float *g_x, *g_h, *partials;
};

// the wave's four Wh^T fragments of k-step ks (hidden-column tiles 4 wave + i).  wht: the image + the wave's tile, uniform
__device__ __forceinline__ void fetch_wht(bf16x8 (&b)[4], const char* __restrict__ wht, uint32_t lane16, int ks) {
#pragma unroll
  for (int i = 0; i < 4; i++) b[i] = *reinterpret_cast<const bf16x8*>(frag_base(wht + (i * kGK + ks) * (kFrag * 2)) + lane16);
}

// r, u, c, q and h' of one step at this lane's 16 (robot, hidden unit) pairs, [i][r]; rows beyond n read as zero
struct Saved {
  float r[4][4], u[4][4], c[4][4], q[4][4], h[4][4];
  __device__ __forceinline__ void load(const BwdParams& P, int t, int row0, int r0, int wave, int col) {
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
      const int robot = row0 + r0 + rr;
      const bool live = robot < P.n;
      const size_t o = (size_t)t * P.n + (live ? robot : 0);
      const float* sv = row_base(P.saved + o * (4 * kHid) + 64 * wave + col);
      const float* hp = row_base(P.hprev + o * kHid + 64 * wave + col);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float vr = sv[16 * i], vu = sv[kHid + 16 * i], vc = sv[2 * kHid + 16 * i], vq = sv[3 * kHid + 16 * i], vh = hp[16 * i];
        r[i][rr] = live ? vr : 0.0f; u[i][rr] = live ? vu : 0.0f; c[i][rr] = live ? vc : 0.0f;     // loads of robot 0's row, then a select:
        q[i][rr] = live ? vq : 0.0f; h[i][rr] = live ? vh : 0.0f;                                 // no branch per element
      }
    }
  }
};

__global__ __launch_bounds__(256) void gru_backward_bf16_kernel(BwdParams P) {
  __shared__ __attribute__((aligned(16))) __bf16 s_g[2][kRows * kGS];
  __shared__ __attribute__((aligned(16))) __bf16 s_l[2][kRows * kLS];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;      // wave: uniform, in an SGPR
  const int row0 = blockIdx.x * kRows;
  const int col = lane & 15, r0 = 4 * (lane >> 4);
  const size_t n = (size_t)P.n;
  // Wo^T's share of the wave, resident; the Wh^T ring: the first seven k-steps of the first contraction
  bf16x8 wo[4][kLK / 32];
  {
    const bf16x8* wot = reinterpret_cast<const bf16x8*>(P.wot) + (size_t)(4 * wave) * (kLK / 32) * 64 + lane;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int ks = 0; ks < kLK / 32; ks++) wo[i][ks] = wot[(i * (kLK / 32) + ks) * 64];
  }
  const char* wht = reinterpret_cast<const char*>(P.wht) + (size_t)(4 * wave) * kGK * (kFrag * 2);
  const uint32_t lane16 = 16 * lane;
  bf16x8 ring[kBwdDepth][4];
  if (P.T > 1) {
#pragma unroll
    for (int d = 0; d < kBwdDepth - 1; d++) fetch_wht(ring[d], wht, lane16, d);
  }
  constexpr int kLoads = kRows * kLat / 256;      // the loader's share of a g_latent tile: three words
  static_assert(kLoads * 256 == kRows * kLat, "whole words per thread");
  Saved sv;
  sv.load(P, P.T - 1, row0, r0, wave, col);
  {
    const int t = P.T - 1;
    const __bf16 z = (__bf16)0.0f;
#pragma unroll
    for (int e = 0; e < 2; e++) {                 // the 16 zero columns behind the 48 of a g_latent tile, both buffers: written once
      const int i = tid + 256 * e, b = i >> 8, r = (i >> 4) & 15, c = kLat + (i & 15);
      s_l[b][r * kLS + c] = z;
    }
#pragma unroll
    for (int e = 0; e < kLoads; e++) {
      const int i = tid + 256 * e, r = i / kLat, c = i - r * kLat;
      s_l[t & 1][r * kLS + c] = (__bf16)(row0 + r < P.n ? P.g_latent[((size_t)t * n + row0 + r) * kLat + c] : 0.0f);
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
    bool start_c[4];
#pragma unroll
    for (int r = 0; r < 4; r++) start_c[r] = (row0 + r0 + r < P.n) ? P.starts[(size_t)t * n + row0 + r0 + r] != 0 : true;
    {
      const __bf16* arow = s_l[cur] + col * kLS + 8 * (lane >> 4);
#pragma unroll
      for (int ks = 0; ks < kLK / 32; ks++) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(arow + 32 * ks);
#pragma unroll
        for (int i = 0; i < 4; i++) dh[i] = mfma(a, wo[i][ks], dh[i]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = r0 + r, robot = row0 + row;
      const bool live = robot < P.n;
      const size_t o = ((size_t)t * n + (live ? robot : 0)) * kGates + 64 * wave + col;
      float* gx = row_base(P.g_x + o);
      float* gh = row_base(P.g_h + o);
      __bf16* g = s_g[cur] + row * kGS + 64 * wave + col;
      float vr[4], vu[4], vc[4], vg[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float d = dh[i][r], rr = sv.r[i][r], uu = sv.u[i][r], c = sv.c[i][r], q = sv.q[i][r];
        const float du = d * (sv.h[i][r] - c), dc = d * (1.0f - uu);
        const float dcp = dc * (1.0f - c * c), dup = du * uu * (1.0f - uu);
        const float drp = dcp * q * rr * (1.0f - rr), gc = rr * dcp;
        g[16 * i] = (__bf16)drp; g[kHid + 16 * i] = (__bf16)dup; g[2 * kHid + 16 * i] = (__bf16)gc;
        vr[i] = drp; vu[i] = dup; vc[i] = dcp; vg[i] = gc;
        sr[i] += drp; su[i] += dup; sc[i] += dcp; sq[i] += gc;
        dh[i][r] = uu * d;
      }
      if (live) {                                 // the row's stores behind one branch
#pragma unroll
        for (int i = 0; i < 4; i++) {
          gx[16 * i] = vr[i]; gx[kHid + 16 * i] = vu[i]; gx[2 * kHid + 16 * i] = vc[i];
          gh[16 * i] = vr[i]; gh[kHid + 16 * i] = vu[i]; gh[2 * kHid + 16 * i] = vg[i];
        }
      }
    }
    if (t == 0) break;                            // no gradient with respect to h0
#pragma unroll
    for (int e = 0; e < kLoads; e++) {
      const int i = tid + 256 * e, r = i / kLat, c = i - r * kLat;
      s_l[nxt][r * kLS + c] = (__bf16)gl[e];
    }
    __syncthreads();
    sv.load(P, t - 1, row0, r0, wave, col);       // the next step's saved values: under this step's contraction
    const bool more = t > 1;                      // step t - 1 contracts as well: keep the ring turning
    const __bf16* arow = s_g[cur] + col * kGS + 8 * (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < kGK; ks++) {
      if (ks + kBwdDepth - 1 < kGK || more) fetch_wht(ring[(ks + kBwdDepth - 1) % kBwdDepth], wht, lane16, (ks + kBwdDepth - 1) % kGK);
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(arow + 32 * ks);
#pragma unroll
      for (int i = 0; i < 4; i++) dh[i] = mfma(a, ring[ks % kBwdDepth][i], dh[i]);
      __builtin_amdgcn_sched_barrier(0);          // keep the ring as written: no request moves up across a k-step
    }
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

inline int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? orr_fail(-2, who, e) : 0;
}

}  // namespace

extern "C" {

int64_t orr_gru_packed_bf16_size(int32_t k, int32_t n) {
  if (k <= 0 || n <= 0) return -1;
  return (int64_t)((n + 15) / 16) * ((k + 31) / 32) * kFrag;
}

int32_t orr_gru_pack_bf16(const float* w, int32_t k, int32_t n, int32_t transpose, uint16_t* out, void* stream) {
  const long long size = transpose ? orr_gru_packed_bf16_size(n, k) : orr_gru_packed_bf16_size(k, n);
  if (!w || !out || size < 0) return orr_fail(-1, "orr_gru_pack_bf16: bad argument", hipSuccess);
  if (misaligned(w, 3) || misaligned(out, 15)) return orr_fail(-1, "orr_gru_pack_bf16: w must be 4-byte aligned, the image 16-byte aligned", hipSuccess);
  if (overlap(Range{w, (size_t)k * (size_t)n * 4}, Range{out, (size_t)size * 2})) return orr_fail(-1, "orr_gru_pack_bf16: the image overlaps w", hipSuccess);
  const long long total = size / 8;
  hipLaunchKernelGGL(pack_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (int)k, (int)n, (int)(transpose != 0),
                     reinterpret_cast<__bf16*>(out), (int)(((transpose ? n : k) + 31) / 32), total);
  return launched("orr_gru_pack_bf16: launch");
}

int32_t orr_gru_forward_bf16(const orr_gru_encoder_bf16* enc, const float* obs, const uint8_t* starts, const float* h0, int32_t t, int32_t n, float* hid,
                             float* latent, float* frames, float* hprev, float* saved, void* stream) {
  if (!enc || !obs || !hid || t < 1 || n < 1) return orr_fail(-1, "orr_gru_forward_bf16: bad argument", hipSuccess);
  if (!starts && t != 1) return orr_fail(-1, "orr_gru_forward_bf16: starts == NULL (everybody starts) goes with T = 1 only", hipSuccess);
  const void* const p[6] = {enc->wx, enc->bx, enc->wh, enc->bh, enc->wo, enc->bo};
  for (int i = 0; i < 6; i++) {
    if (!p[i]) return orr_fail(-1, "orr_gru_forward_bf16: orr_gru_encoder_bf16 has a null pointer", hipSuccess);
    if (misaligned(p[i], i % 2 == 0 ? 15 : 3))     // images are read 16 bytes per lane
      return orr_fail(-1, "orr_gru_forward_bf16: images must be 16-byte aligned, biases 4-byte aligned", hipSuccess);
  }
  if (misaligned(hid, 15) || misaligned(saved, 15)) return orr_fail(-1, "orr_gru_forward_bf16: hid and saved must be 16-byte aligned", hipSuccess);
  for (const void* q : {(const void*)obs, (const void*)h0, (const void*)latent, (const void*)frames, (const void*)hprev})
    if (misaligned(q, 3)) return orr_fail(-1, "orr_gru_forward_bf16: buffers must be 4-byte aligned", hipSuccess);
  const size_t rows = (size_t)t * (size_t)n;
  const Range out[5] = {{hid, rows * kHid * 4}, {latent, rows * kLat * 4}, {frames, rows * kFrame * 4}, {hprev, rows * kHid * 4},
                        {saved, rows * 4 * kHid * 4}};
  if (any_overlap(out)) return orr_fail(-1, "orr_gru_forward_bf16: outputs overlap", hipSuccess);
  const Range in[3] = {{obs, rows * kObs * 4}, {starts, rows}, {h0, (size_t)n * kHid * 4}};
  for (int i = 0; i < 5; i++)
    for (int j = 0; j < 3; j++) {
      if (i == 0 && j == 2 && t == 1 && hid == h0) continue;      // the rollout's step in place: every read of a row precedes its writes
      if (overlap(out[i], in[j])) return orr_fail(-1, "orr_gru_forward_bf16: an output overlaps an input (hid may BE h0 with T = 1 only)", hipSuccess);
    }
  FwdParams P;
  P.wx = reinterpret_cast<const __bf16*>(enc->wx); P.wh = reinterpret_cast<const __bf16*>(enc->wh); P.wo = reinterpret_cast<const __bf16*>(enc->wo);
  P.bx = enc->bx; P.bh = enc->bh; P.bo = enc->bo;
  P.obs = obs; P.starts = starts; P.h0 = h0; P.T = t; P.n = n;
  P.hid = hid; P.latent = latent; P.frames = frames; P.hprev = hprev; P.saved = saved;
  hipLaunchKernelGGL(gru_forward_bf16_kernel, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(256), 0, (hipStream_t)stream, P);
  return launched("orr_gru_forward_bf16: launch");
}

int32_t orr_gru_backward_bf16(const orr_gru_transposed_bf16* enc, const float* g_latent, const float* saved, const float* hprev, const uint8_t* starts,
                              int32_t t, int32_t n, float* g_x, float* g_h, float* partials, void* stream) {
  if (!enc || !enc->wht || !enc->wot || !g_latent || !saved || !hprev || !starts || !g_x || !g_h || !partials || t < 1 || n < 1)
    return orr_fail(-1, "orr_gru_backward_bf16: bad argument", hipSuccess);
  if (misaligned(enc->wht, 15) || misaligned(enc->wot, 15) || misaligned(saved, 15) || misaligned(g_x, 15) || misaligned(g_h, 15))
    return orr_fail(-1, "orr_gru_backward_bf16: images, saved, g_x and g_h must be 16-byte aligned", hipSuccess);
  for (const void* q : {(const void*)g_latent, (const void*)hprev, (const void*)partials})
    if (misaligned(q, 3)) return orr_fail(-1, "orr_gru_backward_bf16: buffers must be 4-byte aligned", hipSuccess);
  const size_t rows = (size_t)t * (size_t)n;
  const Range out[3] = {{g_x, rows * kGates * 4}, {g_h, rows * kGates * 4}, {partials, (size_t)ORR_GRU_BACKWARD_PARTIAL_FLOATS(n) * 4}};
  if (any_overlap(out)) return orr_fail(-1, "orr_gru_backward_bf16: outputs overlap", hipSuccess);
  const Range in[4] = {{g_latent, rows * kLat * 4}, {saved, rows * 4 * kHid * 4}, {hprev, rows * kHid * 4}, {starts, rows}};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++)
      if (overlap(out[i], in[j])) return orr_fail(-1, "orr_gru_backward_bf16: an output overlaps an input", hipSuccess);
  BwdParams P;
  P.wht = reinterpret_cast<const __bf16*>(enc->wht); P.wot = reinterpret_cast<const __bf16*>(enc->wot);
  P.g_latent = g_latent; P.saved = saved; P.hprev = hprev; P.starts = starts; P.T = t; P.n = n;
  P.g_x = g_x; P.g_h = g_h; P.partials = partials;
  hipLaunchKernelGGL(gru_backward_bf16_kernel, dim3((unsigned)ORR_GRU_BACKWARD_ROWS(n)), dim3(256), 0, (hipStream_t)stream, P);
  return launched("orr_gru_backward_bf16: launch");
}

}  // extern "C"
