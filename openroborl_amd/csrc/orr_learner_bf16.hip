// orr_learner_bf16.hip -- the hidden layers' contractions of the PPO update on the bf16 matrix cores (include/openroborl_learner.h:
// orr_dense_forward_bf16, orr_dgrad_relu_bf16, orr_wgrad_bf16; host side: learner_hip._FusedLearner(bf16_gemm=True)).  A translation unit of
// its own: every other kernel of the library compiles exactly as it did.  Mixed precision in the usual sense: every global buffer is float32,
// operands are rounded to bf16 (round to nearest even, v_cvt_pk_bf16_f32) on their way into LDS, products accumulate in f32 registers on
// v_mfma_f32_16x16x32_bf16, and bias, ReLU, masks and every partial sum stay f32.  No bf16 copy of anything lives in HBM, no cast launch.
//
// One tile core (contract) for the three: C[i][j] = sum over t of A[i][t] B[j][t].  BOTH operands lie in LDS as bf16 rows along the
// contraction index t, whatever their layout in memory, so that the fragment of a k-step - eight consecutive t per lane - is ONE ds_read_b128
// at row l & 15, t = 32 step + 8 (l >> 4), for A and for B alike (the instruction pairs element e of lane group l >> 4 of A with the same
// element of B: any order of t that both sides share is a correct contraction).  D: register r of lane l is C[4 (l >> 4) + r][l & 15].
//   workgroup   256 threads = 4 waves (2 x 2); forward and dgrad: 64 batch rows x 128 columns, a wave owns 32 x 64 = 2 x 4 MFMA tiles (32
//               accumulator registers), the geometry of the two f32 siblings (orr_dgrad_partial_rows serves both dgrads); wgrad: 64 x 64 of gw x
//               one batch slice, a wave owns 2 x 2 tiles
//   chunk       KC = 64 t per chunk = two k-steps of 32, two buffers: a thread issues the global loads of chunk c + 1, runs the MFMAs of
//               chunk c, then rounds and stores the loads into the other buffer: one barrier per chunk.  Per chunk and wave 12 ds_read_b128
//               for 16 MFMAs (forward, dgrad), each MFMA doing the work of eight of the f32 kernels'
//   LDS stride  64 + 8 bf16 = 36 words: the 16 rows of a quad start 4 banks apart mod 64 (36 r mod 64 runs through the multiples of 4), so a
//               quad's 16-byte reads cover the 64 banks once; 55296 bytes (forward, dgrad) and 36864 bytes (wgrad): two workgroups per CU
//   Rows        operands whose t is contiguous in memory (x in forward, gz and W in dgrad): a 16-byte granule of four t is rounded to four
//               bf16 and stored with one ds_write_b64; 16 lanes fill a row, a wave's four rows hit every bank twice (the least for 512 bytes)
//   Cols        operands whose t is the row index in memory (W in forward, x and g in wgrad): transposed IN THE STAGE.  A thread loads a
//               4 (t) x 4 (j) block as four 16-byte granules of four consecutive memory rows; column jj of the block is four consecutive t of
//               LDS row j + jj - the transpose is a choice of registers, no data moves - and goes out as one ds_write_b64: as many loads
//               and stores as Rows.  A wave covers 8 j-blocks x 8 t-blocks: 128 contiguous bytes per memory row, and its stores hit every
//               bank twice (16 jg + 2 tg mod 64 words)
//   tails       a granule or block beyond the contraction length, beyond m or beyond the matrix is replaced by zeros in LDS, never read
//               (k = 208 = 3 chunks + 16, n = 48, m no multiple of 64); the second k-step of a chunk with at most 32 t left is skipped, and a
//               wave skips the MFMA tiles outside the matrix and stores none of them (n = 48, k = 160 / 208 against 64-wide wgrad tiles)
//   forward     the gathers and the xa | xb concatenation in the A loader as in orr_dense_forward (row numbers read once, pointers kept);
//               column block 0 writes the f32 granules it loaded to x_out - before rounding, bit for bit; epilogue acc + b, ReLU
//   dgrad       epilogue as orr_dgrad_relu: the f32 h at the accumulators' coordinates, +0 where h <= 0, column sums lane -> LDS -> one
//               thread per column in a fixed order, one row of ws per 64 batch rows
//   wgrad       slices as orr_wgrad: S = min(16, ceil(512 / tiles), ceil(m / 128)), a slice is ceil(m / S) rows rounded up to whole chunks of
//               64, the last slices may be short or empty (zeros)
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950), no scratch anywhere:
//   forward_kernel   132 VGPRs + 32 AGPRs, LDS 55296 bytes, 2 waves per SIMD
//   dgrad_kernel     124 VGPRs + 32 AGPRs, LDS 59392 bytes (the column sums' 4 KB included), 2 waves per SIMD
//   wgrad_kernel      86 VGPRs + 16 AGPRs, LDS 36864 bytes, 4 waves per SIMD
// Measured (profiles/bf16_gemm.txt, m = 16384, library / f32 HIP / this): 512 -> 256 36.0 / 48.6 / 21.5 us, gather + 160 -> 512 38.0 / 40.4 /
// 25.5, the weight gradients 29 .. 41 / 55 .. 56 / 24 .. 30, the input gradient 256 -> 512 59.5 / 63.3 / 38.0; the PPO update 7.70 -> 5.99 ms per
// iteration.  Error against the rounded operands contracted in float64: at most 0.05 of 2 (t + 2) 2^-24 S (tests/test_gpu_learner_bf16.py).
// Tried and dropped / not tried: the transposing LDS read (ds_read_b64_tr_b16 on operands stored as they lie) was NOT built - the register
// transpose above costs no instruction beyond the conversions the stage needs anyway, and keeps one fragment read for both operand kinds;
// 128 x 128 tiles (256 workgroups at 512 -> 256, m = 16384: one wave per SIMD on a kernel that waits for memory, and orr_dgrad_partial_rows
// would no longer serve).
// No atomics; every order is a function of the shape.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/openroborl_learner.h"

int orr_fail(int code, const char* msg, hipError_t e);  // orr_kernels.hip

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kThreads = 256;
constexpr int KC = 64, S = KC + 8;          // contraction indices per chunk; LDS row stride, both in bf16
constexpr int kRows = 64, kCols = 128;      // forward and dgrad: the workgroup's tile
constexpr int kWgTile = 64, kWgMaxSlices = 16, kWgGroups = 512, kWgMinRows = 128;

__device__ __forceinline__ void put4(__bf16* d, float a, float b, float c, float e) {       // round to nearest even, one 8-byte store
  *reinterpret_cast<bf16x4*>(d) = bf16x4{(__bf16)a, (__bf16)b, (__bf16)c, (__bf16)e};
}

// An operand whose contraction index is contiguous in memory: src [nrows][T], rows row0 .. row0 + R - 1 of it.
template <int R>
struct Rows {
  static constexpr int P = R * (KC / 4) / kThreads;
  const float* src;
  int row0, nrows, T, tid;
  f32x4 v[P];
  __device__ __forceinline__ void fetch(long long t0) {
#pragma unroll
    for (int p = 0; p < P; p++) {
      const int idx = tid + kThreads * p, row = row0 + idx / 16, t = (int)t0 + 4 * (idx % 16);
      v[p] = (row < nrows && t < T) ? *reinterpret_cast<const f32x4*>(src + (size_t)row * T + t) : f32x4{0, 0, 0, 0};
    }
  }
  __device__ __forceinline__ void stage(__bf16* lds, long long) {
#pragma unroll
    for (int p = 0; p < P; p++) {
      const int idx = tid + kThreads * p;
      put4(lds + (idx / 16) * S + 4 * (idx % 16), v[p][0], v[p][1], v[p][2], v[p][3]);
    }
  }
};

// The forward pass's input: in(i) = xa[ra(i)][0..ka) | xb[rb(i)][0..kb), 64 rows; the granules go to x_out as they were loaded.
struct Gather {
  static constexpr int P = kRows * (KC / 4) / kThreads;
  const float *pa[P], *pb[P];   // this thread's source rows; NULL: a row beyond m
  float* po[P];                 // its rows of x_out; NULL: not this workgroup's to write
  f32x4 v[P];
  int ka, K, tid;
  __device__ __forceinline__ void init(const float* xa, const int64_t* ra, int ka_, const float* xb, const int64_t* rb, int kb, int i0, int M,
                                       float* x_out, int tid_) {
    ka = ka_; K = ka_ + kb; tid = tid_;
#pragma unroll
    for (int p = 0; p < P; p++) {
      const int row = i0 + (tid + kThreads * p) / 16;
      pa[p] = pb[p] = nullptr; po[p] = nullptr;
      if (row < M) {
        pa[p] = xa + (size_t)(ra ? ra[row] : (int64_t)row) * ka;
        if (xb) pb[p] = xb + (size_t)(rb ? rb[row] : (int64_t)row) * kb;
        if (x_out) po[p] = x_out + (size_t)row * K;
      }
    }
  }
  __device__ __forceinline__ void fetch(long long t0) {
#pragma unroll
    for (int p = 0; p < P; p++) {
      const int t = (int)t0 + 4 * ((tid + kThreads * p) % 16);
      v[p] = f32x4{0, 0, 0, 0};
      if (pa[p] && t < K) v[p] = *reinterpret_cast<const f32x4*>(t < ka ? pa[p] + t : pb[p] + (t - ka));
    }
  }
  __device__ __forceinline__ void stage(__bf16* lds, long long t0) {
#pragma unroll
    for (int p = 0; p < P; p++) {
      const int idx = tid + kThreads * p, t = (int)t0 + 4 * (idx % 16);
      put4(lds + (idx / 16) * S + 4 * (idx % 16), v[p][0], v[p][1], v[p][2], v[p][3]);
      if (po[p] && t < K) *reinterpret_cast<f32x4*>(po[p] + t) = v[p];
    }
  }
};

// An operand whose contraction index is the ROW index in memory: src [t_end][ld], columns j0 .. j0 + R - 1 of it (those below nj exist).
// LDS row j holds column j0 + j: the transpose is the choice of registers in stage().
template <int R>
struct Cols {
  static constexpr int P = R / 64;          // 4 x 4 blocks per thread
  const float* src;
  int ld, j0, nj, tid;
  long long t_end;
  f32x4 v[P][4];
  __device__ __forceinline__ int jg(int p) const { return (tid & 7) + 8 * (((tid >> 6) & 1) + 2 * p); }
  __device__ __forceinline__ int tg() const { return ((tid >> 3) & 7) + 8 * (tid >> 7); }
  __device__ __forceinline__ void fetch(long long t0) {
#pragma unroll
    for (int p = 0; p < P; p++) {
      const int j = j0 + 4 * jg(p);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const long long t = t0 + 4 * tg() + e;
        v[p][e] = (j < nj && t < t_end) ? *reinterpret_cast<const f32x4*>(src + (size_t)t * ld + j) : f32x4{0, 0, 0, 0};
      }
    }
  }
  __device__ __forceinline__ void stage(__bf16* lds, long long) {
#pragma unroll
    for (int p = 0; p < P; p++)
#pragma unroll
      for (int jj = 0; jj < 4; jj++) put4(lds + (4 * jg(p) + jj) * S + 4 * tg(), v[p][0][jj], v[p][1][jj], v[p][2][jj], v[p][3][jj]);
  }
};

// acc[ta][tb] += the 16 x 16 tiles (wm + 16 ta, wn + 16 tb) of A B^T over t in [t_begin, t_begin + T), for ta < na and tb < nb.
// as, bs: two buffers of RA x S and RB x S bf16.  Every thread of the workgroup calls it (barriers inside).
template <int TA, int TB, int RA, int RB, class LA, class LB>
__device__ __forceinline__ void contract(LA& A, LB& B, __bf16* as, __bf16* bs, long long t_begin, int T, int na, int nb, int wm, int wn, int lane,
                                         f32x4 (&acc)[TA][TB]) {
  const int nchunks = (T + KC - 1) / KC;
#pragma unroll
  for (int ta = 0; ta < TA; ta++)
#pragma unroll
    for (int tb = 0; tb < TB; tb++) acc[ta][tb] = f32x4{0, 0, 0, 0};
  if (nchunks > 0) {
    A.fetch(t_begin);
    B.fetch(t_begin);
    A.stage(as, t_begin);
    B.stage(bs, t_begin);
  }
  __syncthreads();
  const int afrag = (wm + (lane & 15)) * S + 8 * (lane >> 4), bfrag = (wn + (lane & 15)) * S + 8 * (lane >> 4);
  for (int c = 0; c < nchunks; c++) {
    const int buf = c & 1;
    const bool more = c + 1 < nchunks;
    const long long t_next = t_begin + (long long)(c + 1) * KC;
    if (more) {
      A.fetch(t_next);
      B.fetch(t_next);
    }
    const __bf16* ap = as + buf * RA * S + afrag;
    const __bf16* bp = bs + buf * RB * S + bfrag;
    const int nsteps = T - c * KC > 32 ? 2 : 1;      // a last chunk of at most 32: its second k-step holds zeros only
#pragma unroll
    for (int ks = 0; ks < KC / 32; ks++)
      if (ks < nsteps) {
        bf16x8 a[TA], b[TB];
#pragma unroll
        for (int t = 0; t < TA; t++) a[t] = *reinterpret_cast<const bf16x8*>(ap + 16 * t * S + 32 * ks);
#pragma unroll
        for (int t = 0; t < TB; t++) b[t] = *reinterpret_cast<const bf16x8*>(bp + 16 * t * S + 32 * ks);
#pragma unroll
        for (int ta = 0; ta < TA; ta++)
#pragma unroll
          for (int tb = 0; tb < TB; tb++)
            if (ta < na && tb < nb) acc[ta][tb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
      }
    if (more) {                              // the buffers chunk c - 1 was read from: every wave has passed the barrier behind it
      A.stage(as + (buf ^ 1) * RA * S, t_next);
      B.stage(bs + (buf ^ 1) * RB * S, t_next);
    }
    __syncthreads();
  }
}

// ---- orr_dense_forward_bf16 -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void forward_kernel(const float* __restrict__ xa, const int64_t* __restrict__ ra, int ka,
                                                           const float* __restrict__ xb, const int64_t* __restrict__ rb, int kb, int M,
                                                           const float* __restrict__ w, const float* __restrict__ b, int N, int relu,
                                                           float* __restrict__ y, float* __restrict__ x_out) {
  __shared__ __attribute__((aligned(16))) __bf16 as[2 * kRows * S];
  __shared__ __attribute__((aligned(16))) __bf16 bs[2 * kCols * S];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * kRows, c0 = blockIdx.y * kCols;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 64;
  const int nb = max(0, min(4, (N - c0 - wn) / 16));
  Gather A;
  A.init(xa, ra, ka, xb, rb, kb, i0, M, blockIdx.y == 0 ? x_out : nullptr, tid);
  Cols<kCols> B = {w, N, c0, N, tid, (long long)(ka + kb)};
  f32x4 acc[2][4];
  contract<2, 4, kRows, kCols>(A, B, as, bs, 0, ka + kb, 2, nb, wm, wn, lane, acc);
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
          const float z = acc[ta][tb][r] + bias;
          if (row < M) y[(size_t)row * N + col] = relu ? fmaxf(z, 0.0f) : z;
        }
    }
}

// ---- orr_dgrad_relu_bf16 --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dgrad_kernel(const float* __restrict__ gz, const float* __restrict__ w, const float* __restrict__ h, int M,
                                                         int N, int K, float* __restrict__ gh, float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) __bf16 as[2 * kRows * S];
  __shared__ __attribute__((aligned(16))) __bf16 bs[2 * kCols * S];
  __shared__ float red[2][4][kCols];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * kRows, c0 = blockIdx.y * kCols;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 64;
  const int nb = max(0, min(4, (K - c0 - wn) / 16));
  Rows<kRows> A = {gz, i0, M, N, tid};
  Rows<kCols> B = {w, c0, K, N, tid};
  f32x4 acc[2][4];
  contract<2, 4, kRows, kCols>(A, B, as, bs, 0, N, 2, nb, wm, wn, lane, acc);
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
  if (tid < kCols && c0 + tid < K) {
    float t = 0.0f;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int e = 0; e < 4; e++) t += red[a][e][tid];
    ws[(size_t)blockIdx.x * K + c0 + tid] = t;
  }
}

// ---- orr_wgrad_bf16 -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wgrad_kernel(const float* __restrict__ x, int K, const float* __restrict__ g, int N, int M,
                                                         long long slice_rows, float* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) __bf16 as[2 * kWgTile * S];
  __shared__ __attribute__((aligned(16))) __bf16 bs[2 * kWgTile * S];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * kWgTile, k0 = blockIdx.y * kWgTile;
  const int wk = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const long long r_begin = (long long)blockIdx.z * slice_rows;
  const long long r_end = r_begin + slice_rows < M ? r_begin + slice_rows : M;
  const int na = max(0, min(2, (K - k0 - wk) / 16)), nb = max(0, min(2, (N - n0 - wn) / 16));
  Cols<kWgTile> A = {x, K, k0, K, tid, r_end};
  Cols<kWgTile> B = {g, N, n0, N, tid, r_end};
  f32x4 acc[2][2];
  contract<2, 2, kWgTile, kWgTile>(A, B, as, bs, r_begin, r_end > r_begin ? (int)(r_end - r_begin) : 0, na, nb, wk, wn, lane, acc);
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

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool dims_ok(int a, int b) { return a >= 16 && b >= 16 && (a % 16) == 0 && (b % 16) == 0; }

// [p, p + bytes) against [q, q + qbytes); a NULL q is no range
inline bool overlaps(const void* p, size_t bytes, const void* q, size_t qbytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), c = reinterpret_cast<uintptr_t>(q);
  return q != nullptr && a < c + qbytes && c < a + bytes;
}

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

int32_t orr_dense_forward_bf16(const float* xa, int32_t ka, const int64_t* rows_a, const float* xb, int32_t kb, const int64_t* rows_b, int32_t m,
                               const float* w, const float* b, int32_t n, int32_t relu, float* y, float* x_out, void* stream) {
  if (!xa || !w || !b || !y || m < 1) return orr_fail(-1, "orr_dense_forward_bf16: bad argument (xa, w, b and y are required, m >= 1)", hipSuccess);
  if (ka < 16 || (ka % 16) != 0 || kb < 0 || (kb % 16) != 0 || n < 16 || (n % 16) != 0)
    return orr_fail(-1, "orr_dense_forward_bf16: ka >= 16 and kb must be multiples of 16, n a multiple of 16 (the output layers are orr_dense_forward's)",
                    hipSuccess);
  if ((xb != nullptr) != (kb > 0) || (rows_b && !xb))
    return orr_fail(-1, "orr_dense_forward_bf16: xb and kb come together (and rows_b with them)", hipSuccess);
  if (misaligned(xa, 16) || misaligned(xb, 16) || misaligned(w, 16) || misaligned(y, 16) || misaligned(x_out, 16) || misaligned(b, 4) ||
      misaligned(rows_a, 8) || misaligned(rows_b, 8))
    return orr_fail(-1, "orr_dense_forward_bf16: xa, xb, w, y and x_out must be 16-byte aligned, b and the row tables to their element size", hipSuccess);
  // the outputs against every input (of a source read through a row table the entry knows no height: its first m rows) and each other
  const size_t f = sizeof(float), k = (size_t)ka + (size_t)kb, rows = (size_t)m;
  const struct { const void* p; size_t bytes; } in[] = {{xa, rows * ka * f}, {xb, rows * kb * f}, {w, k * n * f}, {b, (size_t)n * f},
                                                        {rows_a, rows * sizeof(int64_t)}, {rows_b, rows * sizeof(int64_t)}};
  for (const auto& r : in)
    if (overlaps(y, rows * n * f, r.p, r.bytes) || (x_out && overlaps(x_out, rows * k * f, r.p, r.bytes)))
      return orr_fail(-1, "orr_dense_forward_bf16: y and x_out must not overlap an input", hipSuccess);
  if (x_out && overlaps(x_out, rows * k * f, y, rows * n * f))
    return orr_fail(-1, "orr_dense_forward_bf16: y and x_out must not overlap each other", hipSuccess);
  const dim3 grid((unsigned)(((long long)m + kRows - 1) / kRows), (unsigned)((n + kCols - 1) / kCols));
  if (grid.y > 65535u) return orr_fail(-1, "orr_dense_forward_bf16: n too large", hipSuccess);
  hipLaunchKernelGGL(forward_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, xa, rows_a, (int)ka, xb, rows_b, (int)kb, (int)m, w, b, (int)n,
                     (int)relu, y, x_out);
  return launched("orr_dense_forward_bf16: launch");
}

int32_t orr_dgrad_relu_bf16(const float* gz, const float* w, const float* h, int32_t m, int32_t n, int32_t k, float* gh, float* ws, void* stream) {
  if (!gz || !w || !h || !gh || !ws || m < 1) return orr_fail(-1, "orr_dgrad_relu_bf16: bad argument", hipSuccess);
  if (!dims_ok(k, n)) return orr_fail(-1, "orr_dgrad_relu_bf16: n and k must be multiples of 16", hipSuccess);
  if (misaligned(gz, 16) || misaligned(w, 16) || misaligned(h, 16) || misaligned(gh, 16) || misaligned(ws, 16))
    return orr_fail(-1, "orr_dgrad_relu_bf16: buffers must be 16-byte aligned", hipSuccess);
  const dim3 grid((unsigned)(((long long)m + kRows - 1) / kRows), (unsigned)((k + kCols - 1) / kCols));      // x: orr_dgrad_partial_rows(m)
  if (grid.y > 65535u) return orr_fail(-1, "orr_dgrad_relu_bf16: k too large", hipSuccess);
  hipLaunchKernelGGL(dgrad_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, gz, w, h, (int)m, (int)n, (int)k, gh, ws);
  return launched("orr_dgrad_relu_bf16: launch");
}

int32_t orr_wgrad_bf16_slices(int32_t m, int32_t k, int32_t n) { return wgrad_slices(m, k, n); }

int32_t orr_wgrad_bf16(const float* x, int32_t k, const float* g, int32_t n, int32_t m, float* partials, void* stream) {
  if (!x || !g || !partials || m < 1) return orr_fail(-1, "orr_wgrad_bf16: bad argument", hipSuccess);
  if (!dims_ok(k, n)) return orr_fail(-1, "orr_wgrad_bf16: k and n must be multiples of 16", hipSuccess);
  if (misaligned(x, 16) || misaligned(g, 16) || misaligned(partials, 16)) return orr_fail(-1, "orr_wgrad_bf16: buffers must be 16-byte aligned", hipSuccess);
  const int s = wgrad_slices(m, k, n);
  const long long per = ((long long)m + s - 1) / s;
  const long long slice_rows = (per + KC - 1) / KC * KC;
  const dim3 grid((unsigned)((n + kWgTile - 1) / kWgTile), (unsigned)((k + kWgTile - 1) / kWgTile), (unsigned)s);
  if (grid.y > 65535u) return orr_fail(-1, "orr_wgrad_bf16: k too large", hipSuccess);
  hipLaunchKernelGGL(wgrad_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, x, (int)k, g, (int)n, (int)m, slice_rows, partials);
  return launched("orr_wgrad_bf16: launch");
}

}  // extern "C"
