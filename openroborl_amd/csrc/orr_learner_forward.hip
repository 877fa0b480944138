// orr_learner_forward.hip -- the forward layers of the PPO update on the f32 matrix cores (include/openroborl_learner.h: orr_dense_forward;
// host side: learner_hip._FusedLearner(hip_forward=True)).  A translation unit of its own: every other kernel of the library compiles exactly
// as it did.  y = act(in . W + b) with the minibatch's gathers and the obs | priv concatenation in the loader, and with the ROLLOUT's
// arithmetic: csrc/orr_policy.hip forms every output as one accumulator over k ascending from +0 on v_mfma_f32_16x16x4_f32, k-step j of
// k-group g contracting k = 16 g + 4 j + (0..3), then adds the bias, then takes fmaxf(., 0).  The kernels here issue the same steps in the same
// order on the same instruction, so a learner's forward pass gives the bits the rollout gave for the same weights and inputs.  The layouts:
//   A fragment: lane l holds A[l & 15][l >> 4];  B fragment: lane l holds B[l >> 4][l & 15];  D: register r of lane l is D[4 (l >> 4) + r][l & 15].
//
// dense_kernel (n a multiple of 16): orr_dgrad_relu's shape, which was level with the library at 256 -> 512 (profiles/hip_backward.txt).
//   workgroup   256 threads = 4 waves (2 x 2), 64 batch rows x 128 columns of y; a wave owns 32 x 64 = 2 x 4 MFMA tiles, 32 accumulator
//               registers.  grid = ceil(m / 64) x ceil(n / 128): 1024 workgroups at m = 16384, n = 512
//   stage       KC = 32 contraction columns per chunk (16 where k is no multiple of 32: 208), two buffers; a thread issues the global loads of
//               chunk c + 1, runs the MFMAs of chunk c, then stores the loads into the other buffer: one barrier per chunk
//   A in LDS    the gathered input rows.  orr_dgrad_relu's 16-byte fragment read contracts k in a permuted order, which is not allowed here, so
//               the stage's STORES permute instead (orr_policy_pack's idea applied to the LDS image): a loaded granule x[r][16 g + 4 j + (0..3)]
//               is scattered as four words to r S + 16 g + 4 (0..3) + j, and lane (r, q) reads ONE ds_read_b128 at r S + 16 g + 4 q whose
//               element j is x[r][16 g + 4 j + q], the A operand of k-step j.  S = KC + 4 words: the 16 rows of a quad cover the 64 banks once
//               on the read; the scattered stores are 2-way conflicted (8 rows x 8 granules of a wave) - 4 ds_write_b32 per thread and chunk
//               against 32 MFMAs per wave
//   B in LDS    W as stored, [k][n] row-major, no packing launch (the weights move every optimiser step): KC rows x 128 columns at a stride of
//               128 + 16 words, 16-byte stores; the B fragment of a k-step is a 4-byte read at row 4 j + q, column c: the four rows start 16
//               banks apart, the 64 lanes cover the 64 banks once.  Per k-group and wave: 2 ds_read_b128 + 16 ds_read_b32 for 32 MFMAs
//   gather      a thread loads the same rows of the tile in every chunk: it reads its row numbers from the tables once and keeps the two source
//               pointers; a granule lies in xa or in xb as a whole (ka is a multiple of 16).  The workgroups of column block 0 write the
//               granules they load to x_out on their way to LDS - the layer's input for its weight gradient, written once
//   remainder   n = 48 and rows beyond m: loads outside are replaced by zeros (whole granules), a wave skips the column tiles that lie outside
//               and stores nothing there; k = 160 runs 5 chunks of 32, k = 208 13 chunks of 16 - no k-step is ever padded
// dense_small_kernel (n <= 15: the output layers of fan-out 12 and 1): no GEMM, as orr_head_backward argues, but the rollout's heads run on
// the matrix cores with the missing columns as zeros, and so does this: a wave owns 16 rows and ONE column tile, A staged as above at KC = 16
// (a wave stages exactly its own rows), the B fragment read from global memory, W[k][c] for c < n and +0 beyond (12 KB at 256 x 12: L2 / L1
// hits).  64 dependent MFMAs per wave at k = 256; 256 workgroups at m = 16384.
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950), no scratch anywhere:
//   dense_kernel<32>    72 VGPRs + 32 AGPRs, LDS 55296 bytes (two workgroups of it fit a CU's 160 KB), 2 waves per SIMD
//   dense_kernel<16>    46 VGPRs + 32 AGPRs, LDS 28672 bytes
//   dense_small_kernel  34 VGPRs +  4 AGPRs, LDS 10240 bytes
// Measured (profiles/hip_forward.txt, m = 16384): the gathering layer 0 is level with index_select + the library at 160 -> 512 and 1.3x faster
// at 208 -> 512 (two gathers and a cat saved), the output layers are 1.8x and 2.5x faster, 512 -> 256 is 1.3x SLOWER (48.8 us against 36.5;
// 27 us would be the matrix cores' peak) and that costs the update more than the rest wins.  Tried and dropped: loads two chunks ahead in a
// second register set (110 VGPRs; 48.3 us, no change - the global latency is not what the kernel waits for).
// Rejected before measuring: packing W per call (a launch and a round trip of the weights per layer and step); 4-byte A fragment reads at an odd
// stride (the rollout's choice: 4 LDS reads where one serves); a 16-byte B read (its stage would scatter W's granules 4-way conflicted, and B
// is the operand whose reads are already conflict-free); one workgroup per 16 rows with the weights streamed from L2 (the rollout's mapping:
// 1.7 MB of weights per 16 rows is right for 4096 robots and 4x the traffic of this tiling at 16384).
// No atomics; every order is a function of the shape.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/openroborl_learner.h"

int orr_fail(int code, const char* msg, hipError_t e);  // orr_kernels.hip

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kRows = 64, kCols = 128, kBStride = kCols + 16;

struct Source {                 // in(i) = xa[ra(i)][0..ka) | xb[rb(i)][0..kb)
  const float *xa, *xb;
  const int64_t *ra, *rb;
  int ka, kb;
};

// The A side of both kernels: 64 gathered rows x KC columns per chunk, staged in the permuted image the head comment describes.
template <int KC>
struct RowLoader {
  static constexpr int S = KC + 4, Q = KC / 4, P = kRows * Q / kThreads;    // LDS row stride; granules per row and per thread
  const float *pa[P], *pb[P];   // this thread's source rows; NULL: a row beyond m
  float* po[P];                 // its rows of x_out; NULL: not this workgroup's to write
  f32x4 v[P];
  int ka, tid;

  __device__ __forceinline__ void init(const Source& s, int i0, int M, float* x_out, int tid_) {
    ka = s.ka; tid = tid_;
#pragma unroll
    for (int p = 0; p < P; p++) {
      const int row = i0 + (tid + kThreads * p) / Q;
      pa[p] = pb[p] = nullptr; po[p] = nullptr;
      if (row < M) {
        pa[p] = s.xa + (size_t)(s.ra ? s.ra[row] : (int64_t)row) * s.ka;
        if (s.xb) pb[p] = s.xb + (size_t)(s.rb ? s.rb[row] : (int64_t)row) * s.kb;
        if (x_out) po[p] = x_out + (size_t)row * (s.ka + s.kb);
      }
    }
  }
  __device__ __forceinline__ void fetch(int j0) {
#pragma unroll
    for (int p = 0; p < P; p++) {
      const int col = j0 + 4 * ((tid + kThreads * p) % Q);
      v[p] = f32x4{0, 0, 0, 0};
      if (pa[p]) v[p] = *reinterpret_cast<const f32x4*>(col < ka ? pa[p] + col : pb[p] + (col - ka));
    }
  }
  __device__ __forceinline__ void stage(float* as, int j0) {
#pragma unroll
    for (int p = 0; p < P; p++) {
      const int idx = tid + kThreads * p, gran = idx % Q;
      float* d = as + (idx / Q) * S + 16 * (gran / 4) + (gran % 4);
#pragma unroll
      for (int i = 0; i < 4; i++) d[4 * i] = v[p][i];
      if (po[p]) *reinterpret_cast<f32x4*>(po[p] + j0 + 4 * gran) = v[p];
    }
  }
};

__device__ __forceinline__ float finish(float acc, float bias, int relu) {
  const float z = acc + bias;
  return relu ? fmaxf(z, 0.0f) : z;
}

template <int KC>
__global__ __launch_bounds__(kThreads) void dense_kernel(Source src, int M, const float* __restrict__ w, const float* __restrict__ b, int N, int relu,
                                                         float* __restrict__ y, float* __restrict__ x_out) {
  using Loader = RowLoader<KC>;
  constexpr int S = Loader::S, PB = KC * (kCols / 4) / kThreads;
  __shared__ __attribute__((aligned(16))) float as[2][kRows * S];
  __shared__ __attribute__((aligned(16))) float bs[2][KC * kBStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * kRows, c0 = blockIdx.y * kCols;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 64;
  const int nb = max(0, min(4, (N - c0 - wn) / 16));
  const int nchunks = (src.ka + src.kb) / KC;
  Loader A;
  A.init(src, i0, M, blockIdx.y == 0 ? x_out : nullptr, tid);
  f32x4 pb[PB];
  const int bcol = 4 * (tid & 31), brow = tid >> 5;         // W's loader: rows brow + 8 p of the chunk, the granule at column bcol
  const bool bin = c0 + bcol < N;
  const auto fetch_b = [&](int j0) {
#pragma unroll
    for (int p = 0; p < PB; p++)
      pb[p] = bin ? *reinterpret_cast<const f32x4*>(w + (size_t)(j0 + brow + 8 * p) * N + c0 + bcol) : f32x4{0, 0, 0, 0};
  };
  const auto stage_b = [&](int buf) {
#pragma unroll
    for (int p = 0; p < PB; p++) *reinterpret_cast<f32x4*>(&bs[buf][(brow + 8 * p) * kBStride + bcol]) = pb[p];
  };
  f32x4 acc[2][4];
#pragma unroll
  for (int ta = 0; ta < 2; ta++)
#pragma unroll
    for (int tb = 0; tb < 4; tb++) acc[ta][tb] = f32x4{0, 0, 0, 0};
  A.fetch(0);
  fetch_b(0);
  A.stage(as[0], 0);
  stage_b(0);
  __syncthreads();
  const int afrag = (wm + (lane & 15)) * S + 4 * (lane >> 4);
  const int bfrag = (lane >> 4) * kBStride + wn + (lane & 15);
  for (int c = 0; c < nchunks; c++) {
    const int buf = c & 1;
    const bool more = c + 1 < nchunks;
    if (more) {
      A.fetch((c + 1) * KC);
      fetch_b((c + 1) * KC);
    }
#pragma unroll
    for (int g = 0; g < KC / 16; g++) {
      f32x4 a[2];
#pragma unroll
      for (int t = 0; t < 2; t++) a[t] = *reinterpret_cast<const f32x4*>(&as[buf][afrag + 16 * t * S + 16 * g]);
#pragma unroll
      for (int j = 0; j < 4; j++) {          // k = KC c + 16 g + 4 j + (0..3): ascending
        float bv[4];
#pragma unroll
        for (int t = 0; t < 4; t++) bv[t] = bs[buf][bfrag + (16 * g + 4 * j) * kBStride + 16 * t];
#pragma unroll
        for (int ta = 0; ta < 2; ta++)
#pragma unroll
          for (int tb = 0; tb < 4; tb++)
            if (tb < nb) acc[ta][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ta][j], bv[tb], acc[ta][tb], 0, 0, 0);
      }
    }
    if (more) {                              // the buffers chunk c - 1 was read from: every wave has passed the barrier behind it
      A.stage(as[buf ^ 1], (c + 1) * KC);
      stage_b(buf ^ 1);
    }
    __syncthreads();
  }
  const int q = lane >> 4, lcol = lane & 15;
#pragma unroll
  for (int tb = 0; tb < 4; tb++)
    if (tb < nb) {
      const int col = c0 + wn + 16 * tb + lcol;
      const float bias = b[col];
#pragma unroll
      for (int ta = 0; ta < 2; ta++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = i0 + wm + 16 * ta + 4 * q + r;
          if (row < M) y[(size_t)row * N + col] = finish(acc[ta][tb][r], bias, relu);
        }
    }
}

__global__ __launch_bounds__(kThreads) void dense_small_kernel(Source src, int M, const float* __restrict__ w, const float* __restrict__ b, int N,
                                                               int relu, float* __restrict__ y, float* __restrict__ x_out) {
  constexpr int KC = 16;
  using Loader = RowLoader<KC>;
  constexpr int S = Loader::S;
  __shared__ __attribute__((aligned(16))) float as[2][kRows * S];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * kRows;
  const int q = lane >> 4, col = lane & 15;
  const bool cin = col < N;
  const int nchunks = (src.ka + src.kb) / KC;
  Loader A;
  A.init(src, i0, M, x_out, tid);
  float bv[4], bn[4];
  const auto fetch_b = [&](int j0) {         // the B fragments of the chunk's four k-steps: W[j0 + 4 j + q][col], +0 for the columns W has not
#pragma unroll
    for (int j = 0; j < 4; j++) bn[j] = cin ? w[(size_t)(j0 + 4 * j + q) * N + col] : 0.0f;
  };
  f32x4 acc = {0, 0, 0, 0};
  A.fetch(0);
  fetch_b(0);
  A.stage(as[0], 0);
  __syncthreads();
  const int afrag = (16 * wave + col) * S + 4 * q;
  for (int c = 0; c < nchunks; c++) {
    const int buf = c & 1;
    const bool more = c + 1 < nchunks;
#pragma unroll
    for (int j = 0; j < 4; j++) bv[j] = bn[j];
    if (more) {
      A.fetch((c + 1) * KC);
      fetch_b((c + 1) * KC);
    }
    const f32x4 a = *reinterpret_cast<const f32x4*>(&as[buf][afrag]);
#pragma unroll
    for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bv[j], acc, 0, 0, 0);
    if (more) A.stage(as[buf ^ 1], (c + 1) * KC);
    __syncthreads();
  }
  if (!cin) return;
  const float bias = b[col];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = i0 + 16 * wave + 4 * q + r;
    if (row < M) y[(size_t)row * N + col] = finish(acc[r], bias, relu);
  }
}

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// [p, p + bytes) against [q, q + qbytes); a NULL q is no range
inline bool overlaps(const void* p, size_t bytes, const void* q, size_t qbytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), c = reinterpret_cast<uintptr_t>(q);
  return q != nullptr && a < c + qbytes && c < a + bytes;
}

}  // namespace

extern "C" {

int32_t orr_dense_forward(const float* xa, int32_t ka, const int64_t* rows_a, const float* xb, int32_t kb, const int64_t* rows_b, int32_t m,
                          const float* w, const float* b, int32_t n, int32_t relu, float* y, float* x_out, void* stream) {
  if (!xa || !w || !b || !y || m < 1) return orr_fail(-1, "orr_dense_forward: bad argument (xa, w, b and y are required, m >= 1)", hipSuccess);
  if (ka < 16 || (ka % 16) != 0 || kb < 0 || (kb % 16) != 0 || n < 1 || (n > 15 && (n % 16) != 0))
    return orr_fail(-1, "orr_dense_forward: ka >= 16 and kb must be multiples of 16, n a multiple of 16 or at most 15", hipSuccess);
  if ((xb != nullptr) != (kb > 0) || (rows_b && !xb)) return orr_fail(-1, "orr_dense_forward: xb and kb come together (and rows_b with them)", hipSuccess);
  if (misaligned(xa, 16) || misaligned(xb, 16) || misaligned(w, 16) || misaligned(y, 16) || misaligned(x_out, 16) || misaligned(b, 4) ||
      misaligned(rows_a, 8) || misaligned(rows_b, 8))
    return orr_fail(-1, "orr_dense_forward: xa, xb, w, y and x_out must be 16-byte aligned, b and the row tables to their element size", hipSuccess);
  // the outputs against every input (of a source read through a row table the entry knows no height: its first m rows) and each other
  const size_t f = sizeof(float), k = (size_t)ka + (size_t)kb, rows = (size_t)m;
  const struct { const void* p; size_t bytes; } in[] = {{xa, rows * ka * f}, {xb, rows * kb * f}, {w, k * n * f}, {b, (size_t)n * f},
                                                        {rows_a, rows * sizeof(int64_t)}, {rows_b, rows * sizeof(int64_t)}};
  for (const auto& r : in)
    if (overlaps(y, rows * n * f, r.p, r.bytes) || (x_out && overlaps(x_out, rows * k * f, r.p, r.bytes)))
      return orr_fail(-1, "orr_dense_forward: y and x_out must not overlap an input", hipSuccess);
  if (x_out && overlaps(x_out, rows * k * f, y, rows * n * f)) return orr_fail(-1, "orr_dense_forward: y and x_out must not overlap each other", hipSuccess);
  const dim3 grid((unsigned)(((long long)m + kRows - 1) / kRows), (unsigned)((n + kCols - 1) / kCols));
  if (grid.y > 65535u) return orr_fail(-1, "orr_dense_forward: n too large", hipSuccess);
  const Source src = {xa, xb, rows_a, rows_b, (int)ka, (int)kb};
  hipStream_t st = (hipStream_t)stream;
  if (n <= 15)
    hipLaunchKernelGGL(dense_small_kernel, dim3(grid.x), dim3(kThreads), 0, st, src, (int)m, w, b, (int)n, (int)relu, y, x_out);
  else if ((ka + kb) % 32 == 0)
    hipLaunchKernelGGL(dense_kernel<32>, grid, dim3(kThreads), 0, st, src, (int)m, w, b, (int)n, (int)relu, y, x_out);
  else
    hipLaunchKernelGGL(dense_kernel<16>, grid, dim3(kThreads), 0, st, src, (int)m, w, b, (int)n, (int)relu, y, x_out);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? orr_fail(-2, "orr_dense_forward: launch", e) : 0;
}

}  // extern "C"
