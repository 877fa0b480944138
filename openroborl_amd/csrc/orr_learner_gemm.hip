// orr_learner_gemm.hip -- the backward GEMMs of the PPO update on the f32 matrix cores (include/openroborl_learner.h: orr_wgrad,
// orr_dgrad_relu; host side: learner_hip._FusedLearner(hip_backward=True)).  A translation unit of its own: every other kernel of the
// library compiles exactly as it did.  v_mfma_f32_16x16x4_f32 with f32 accumulators in registers, as csrc/orr_policy.hip; its layouts:
//   A fragment: lane l holds A[l & 15][l >> 4];  B fragment: lane l holds B[l >> 4][l & 15];  D: register r of lane l is D[4 (l >> 4) + r][l & 15].
//
// orr_wgrad: gw [k][n] = x^T g, the contraction over the batch.  For one batch row the 16 columns of x that a tile owns are contiguous and
// so are the 16 columns of g: with the batch row as the contraction index BOTH fragments are "row l >> 4, column l & 15" reads of a
// row-major stage - no transpose anywhere.
//   workgroup   256 threads = 4 waves (2 x 2), one 64 x 64 tile of gw x one batch slice; a wave owns 32 x 32 = 2 x 2 MFMA tiles (16 accumulator
//               registers), so an LDS word feeds two MFMAs: 4 ds_read_b32 per 4 MFMAs
//   stage       32 batch rows x 64 columns of x and of g per chunk, two buffers (40 KB): a thread issues its four 16-byte global loads of
//               chunk c + 1, runs the 32 MFMAs of chunk c, then stores the loads into the other buffer: one barrier per chunk
//   LDS stride  64 + 16 words: the four batch rows a fragment read touches start 16 banks apart, its 64 lanes cover 64 banks once
//   remainder   k = 160, 208 and n = 48 are no multiples of 64: loads beyond the matrix are replaced by zeros (16-byte granules, k and n are
//               multiples of 16, so a granule is inside or outside as a whole), a wave skips the MFMA tiles that lie outside and stores none of them
//   slices      S = min(16, ceil(512 / tiles), ceil(m / 128)): tiles x S is 384 to 512 workgroups for the learners' shapes at m = 16384 (1.5 to 2
//               per CU), a slice is at least 128 rows, and S <= 16 keeps the partials at what the 16 bmm products were (5 MB at 16384 x 160 x 512)
//               and on orr_colsum_finish's thread-per-column path.  A slice is ceil(m / S) rows rounded up to whole chunks: the last may be
//               short or empty (zeros)
// Rejected: 128 x 128 tiles (8 tiles at 160 x 512: S = 32+ to fill the chip, twice the partials; 37 % of the MFMAs of k = 160 on zeros); a
// 16-byte fragment read that hands one lane four output rows (no tile of a remainder could be skipped).
//
// orr_dgrad_relu: gh [m][k] = (gz [m][n] . W^T) * (h > 0), W [k][n] as stored.  Here the contraction index j runs along the rows of both
// operands, so a fragment is "row l & 15, four consecutive j at 4 (l >> 4)": one ds_read_b128 serves four k-steps (step e contracts
// j = 16 g + 4 (l >> 4) + e in both operands).  W is staged as its own rows [c][j]; the transpose is this read pattern.
//   workgroup   4 waves (2 x 2), 64 batch rows x 128 columns of gh; a wave owns 32 x 64 = 2 x 4 MFMA tiles (32 accumulator registers): 6
//               ds_read_b128 per 32 MFMAs
//   stage       KC = 32 contraction columns per chunk (16 where n is no multiple of 32: n = 48), two buffers, the same prefetch / barrier
//               scheme; LDS stride KC + 4 words: 16 consecutive lanes (16 rows, one quad) cover the 64 banks once
//   epilogue    h is read at the accumulators' own coordinates, the masked value stored, and its column sums go lane -> LDS -> one thread
//               per column in a fixed order: ws [row block][k], one row per 64 batch rows, for orr_colsum_finish
// No float atomics; every order is a function of the shape.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/openroborl_learner.h"

int orr_fail(int code, const char* msg, hipError_t e);  // orr_kernels.hip

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;

// ---- orr_wgrad ------------------------------------------------------------------------------------------------------------------------
constexpr int kWgTile = 64, kWgChunk = 32, kWgStride = kWgTile + 16;
constexpr int kWgMaxSlices = 16, kWgGroups = 512, kWgMinRows = 128;

__global__ __launch_bounds__(kThreads) void wgrad_kernel(const float* __restrict__ x, int K, const float* __restrict__ g, int N, int M,
                                                         long long slice_rows, float* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float xs[2][kWgChunk * kWgStride];
  __shared__ __attribute__((aligned(16))) float gs[2][kWgChunk * kWgStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * kWgTile, k0 = blockIdx.y * kWgTile;
  const int wk = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const long long r_begin = (long long)blockIdx.z * slice_rows;
  const long long r_end = r_begin + slice_rows < M ? r_begin + slice_rows : M;
  const int nchunks = r_end > r_begin ? (int)((r_end - r_begin + kWgChunk - 1) / kWgChunk) : 0;
  // the MFMA tiles of this wave that lie inside the matrix
  const int na = max(0, min(2, (K - k0 - wk) / 16)), nb = max(0, min(2, (N - n0 - wn) / 16));
  // the loader: rows lr and lr + 16 of the chunk, the 16-byte granule at column lc of both operands
  const int lr = tid >> 4, lc = (tid & 15) * 4;
  const bool xin = k0 + lc < K, gin = n0 + lc < N;
  f32x4 px[2], pg[2];
  const auto fetch = [&](long long row0) {
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const long long row = row0 + lr + 16 * p;
      const bool ok = row < r_end;
      px[p] = (ok && xin) ? *reinterpret_cast<const f32x4*>(x + (size_t)row * K + k0 + lc) : f32x4{0, 0, 0, 0};
      pg[p] = (ok && gin) ? *reinterpret_cast<const f32x4*>(g + (size_t)row * N + n0 + lc) : f32x4{0, 0, 0, 0};
    }
  };
  const auto stage = [&](int buf) {
#pragma unroll
    for (int p = 0; p < 2; p++) {
      *reinterpret_cast<f32x4*>(&xs[buf][(lr + 16 * p) * kWgStride + lc]) = px[p];
      *reinterpret_cast<f32x4*>(&gs[buf][(lr + 16 * p) * kWgStride + lc]) = pg[p];
    }
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int ta = 0; ta < 2; ta++)
#pragma unroll
    for (int tb = 0; tb < 2; tb++) acc[ta][tb] = f32x4{0, 0, 0, 0};
  if (nchunks > 0) {
    fetch(r_begin);
    stage(0);
  }
  __syncthreads();
  const int frag = (lane >> 4) * kWgStride + (lane & 15);
  for (int c = 0; c < nchunks; c++) {
    const int buf = c & 1;
    const bool more = c + 1 < nchunks;
    if (more) fetch(r_begin + (long long)(c + 1) * kWgChunk);
    const float* xa = &xs[buf][frag + wk];
    const float* gb = &gs[buf][frag + wn];
#pragma unroll
    for (int j = 0; j < kWgChunk / 4; j++) {
      float a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; t++) {
        a[t] = xa[4 * j * kWgStride + 16 * t];
        b[t] = gb[4 * j * kWgStride + 16 * t];
      }
#pragma unroll
      for (int ta = 0; ta < 2; ta++)
#pragma unroll
        for (int tb = 0; tb < 2; tb++)
          if (ta < na && tb < nb) acc[ta][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
    }
    if (more) stage(buf ^ 1);      // the buffer chunk c - 1 was read from: every wave has passed the barrier behind it
    __syncthreads();
  }
  float* out = partials + (size_t)blockIdx.z * K * N;
#pragma unroll
  for (int ta = 0; ta < 2; ta++)
#pragma unroll
    for (int tb = 0; tb < 2; tb++)
      if (ta < na && tb < nb) {
        const int row = k0 + wk + 16 * ta + 4 * (lane >> 4), col = n0 + wn + 16 * tb + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; r++) out[(size_t)(row + r) * N + col] = acc[ta][tb][r];
      }
}

// ---- orr_dgrad_relu -------------------------------------------------------------------------------------------------------------------
constexpr int kDgRows = 64, kDgCols = 128;

template <int KC>
__global__ __launch_bounds__(kThreads) void dgrad_relu_kernel(const float* __restrict__ gz, const float* __restrict__ w,
                                                              const float* __restrict__ h, int M, int N, int K, float* __restrict__ gh,
                                                              float* __restrict__ ws) {
  constexpr int S = KC + 4, Q = KC / 4;             // LDS row stride in words; 16-byte granules per staged row
  constexpr int PA = kDgRows * Q / kThreads, PB = kDgCols * Q / kThreads;      // granules a thread loads per chunk: of gz, of W
  __shared__ __attribute__((aligned(16))) float as[2][kDgRows * S];
  __shared__ __attribute__((aligned(16))) float bs[2][kDgCols * S];
  __shared__ float red[2][4][kDgCols];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * kDgRows, c0 = blockIdx.y * kDgCols;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 64;
  const int nb = max(0, min(4, (K - c0 - wn) / 16));
  const int nchunks = N / KC;
  f32x4 pa[PA], pb[PB];
  const auto fetch = [&](int j0) {
#pragma unroll
    for (int p = 0; p < PA; p++) {
      const int idx = tid + kThreads * p, row = i0 + idx / Q;
      pa[p] = row < M ? *reinterpret_cast<const f32x4*>(gz + (size_t)row * N + j0 + 4 * (idx % Q)) : f32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int p = 0; p < PB; p++) {
      const int idx = tid + kThreads * p, row = c0 + idx / Q;
      pb[p] = row < K ? *reinterpret_cast<const f32x4*>(w + (size_t)row * N + j0 + 4 * (idx % Q)) : f32x4{0, 0, 0, 0};
    }
  };
  const auto stage = [&](int buf) {
#pragma unroll
    for (int p = 0; p < PA; p++) {
      const int idx = tid + kThreads * p;
      *reinterpret_cast<f32x4*>(&as[buf][(idx / Q) * S + 4 * (idx % Q)]) = pa[p];
    }
#pragma unroll
    for (int p = 0; p < PB; p++) {
      const int idx = tid + kThreads * p;
      *reinterpret_cast<f32x4*>(&bs[buf][(idx / Q) * S + 4 * (idx % Q)]) = pb[p];
    }
  };
  f32x4 acc[2][4];
#pragma unroll
  for (int ta = 0; ta < 2; ta++)
#pragma unroll
    for (int tb = 0; tb < 4; tb++) acc[ta][tb] = f32x4{0, 0, 0, 0};
  fetch(0);
  stage(0);
  __syncthreads();
  const int frag = (lane & 15) * S + 4 * (lane >> 4);
  for (int c = 0; c < nchunks; c++) {
    const int buf = c & 1;
    const bool more = c + 1 < nchunks;
    if (more) fetch((c + 1) * KC);
    const float* ap = &as[buf][wm * S + frag];
    const float* bp = &bs[buf][wn * S + frag];
#pragma unroll
    for (int kg = 0; kg < KC / 16; kg++) {
      f32x4 a[2], b[4];
#pragma unroll
      for (int t = 0; t < 2; t++) a[t] = *reinterpret_cast<const f32x4*>(ap + 16 * t * S + 16 * kg);
#pragma unroll
      for (int t = 0; t < 4; t++) b[t] = *reinterpret_cast<const f32x4*>(bp + 16 * t * S + 16 * kg);
#pragma unroll
      for (int e = 0; e < 4; e++)
#pragma unroll
        for (int ta = 0; ta < 2; ta++)
#pragma unroll
          for (int tb = 0; tb < 4; tb++)
            if (tb < nb) acc[ta][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ta][e], b[tb][e], acc[ta][tb], 0, 0, 0);
    }
    if (more) stage(buf ^ 1);
    __syncthreads();
  }
  // the epilogue: mask by h at the accumulators' coordinates, store, and this lane's column sums (2 tiles x 4 rows, in that order)
  float cs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const int q = lane >> 4, lcol = lane & 15;
#pragma unroll
  for (int ta = 0; ta < 2; ta++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = i0 + wm + 16 * ta + 4 * q + r;
      if (row < M) {
#pragma unroll
        for (int tb = 0; tb < 4; tb++)
          if (tb < nb) {
            const size_t o = (size_t)row * K + c0 + wn + 16 * tb + lcol;
            const float v = h[o] > 0.0f ? acc[ta][tb][r] : 0.0f;
            gh[o] = v;
            cs[tb] += v;
          }
      }
    }
#pragma unroll
  for (int tb = 0; tb < 4; tb++) red[wave >> 1][q][wn + 16 * tb + lcol] = cs[tb];
  __syncthreads();
  if (tid < kDgCols && c0 + tid < K) {
    float t = 0.0f;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) t += red[a][b][tid];
    ws[(size_t)blockIdx.x * K + c0 + tid] = t;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool dims_ok(int a, int b) { return a >= 16 && b >= 16 && (a % 16) == 0 && (b % 16) == 0; }

int wgrad_slices(int m, int k, int n) {
  if (m < 1 || !dims_ok(k, n)) return -1;
  const int tiles = ((k + kWgTile - 1) / kWgTile) * ((n + kWgTile - 1) / kWgTile);
  const int fill = (kWgGroups + tiles - 1) / tiles, tall = (int)(((long long)m + kWgMinRows - 1) / kWgMinRows);
  const int s = min(kWgMaxSlices, min(fill, tall));
  return s < 1 ? 1 : s;
}

int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? orr_fail(-2, who, e) : 0;
}

}  // namespace

extern "C" {

int32_t orr_wgrad_slices(int32_t m, int32_t k, int32_t n) { return wgrad_slices(m, k, n); }

int32_t orr_wgrad(const float* x, int32_t k, const float* g, int32_t n, int32_t m, float* partials, void* stream) {
  if (!x || !g || !partials || m < 1) return orr_fail(-1, "orr_wgrad: bad argument", hipSuccess);
  if (!dims_ok(k, n)) return orr_fail(-1, "orr_wgrad: k and n must be multiples of 16", hipSuccess);
  if (!aligned16(x) || !aligned16(g) || !aligned16(partials)) return orr_fail(-1, "orr_wgrad: buffers must be 16-byte aligned", hipSuccess);
  const int s = wgrad_slices(m, k, n);
  const long long per = ((long long)m + s - 1) / s;
  const long long slice_rows = (per + kWgChunk - 1) / kWgChunk * kWgChunk;
  const dim3 grid((unsigned)((n + kWgTile - 1) / kWgTile), (unsigned)((k + kWgTile - 1) / kWgTile), (unsigned)s);
  if (grid.y > 65535u) return orr_fail(-1, "orr_wgrad: k too large", hipSuccess);
  hipLaunchKernelGGL(wgrad_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, x, (int)k, g, (int)n, (int)m, slice_rows, partials);
  return launched("orr_wgrad: launch");
}

int32_t orr_dgrad_partial_rows(int32_t m) { return m > 0 ? (int32_t)(((long long)m + kDgRows - 1) / kDgRows) : -1; }

int32_t orr_dgrad_relu(const float* gz, const float* w, const float* h, int32_t m, int32_t n, int32_t k, float* gh, float* ws, void* stream) {
  if (!gz || !w || !h || !gh || !ws || m < 1) return orr_fail(-1, "orr_dgrad_relu: bad argument", hipSuccess);
  if (!dims_ok(k, n)) return orr_fail(-1, "orr_dgrad_relu: n and k must be multiples of 16", hipSuccess);
  if (!aligned16(gz) || !aligned16(w) || !aligned16(h) || !aligned16(gh) || !aligned16(ws))
    return orr_fail(-1, "orr_dgrad_relu: buffers must be 16-byte aligned", hipSuccess);
  const dim3 grid((unsigned)orr_dgrad_partial_rows(m), (unsigned)((k + kDgCols - 1) / kDgCols));
  if (grid.y > 65535u) return orr_fail(-1, "orr_dgrad_relu: k too large", hipSuccess);
  hipStream_t st = (hipStream_t)stream;
  if (n % 32 == 0)
    hipLaunchKernelGGL(dgrad_relu_kernel<32>, grid, dim3(kThreads), 0, st, gz, w, h, (int)m, (int)n, (int)k, gh, ws);
  else
    hipLaunchKernelGGL(dgrad_relu_kernel<16>, grid, dim3(kThreads), 0, st, gz, w, h, (int)m, (int)n, (int)k, gh, ws);
  return launched("orr_dgrad_relu: launch");
}

}  // extern "C"
