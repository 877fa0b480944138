// orr_probe_solver.hip -- TEST-ONLY probe of the constraint solver's two register stages (tests/probe_solver_lib.py,
// tests/test_gpu_solver_primitives.py): delassus_columns<HAS_B> and pgs_sweeps<HAS_B> of csrc/orr_physics.h, called with inputs the
// test chooses.  Both take their operands in registers (Row, ContactGeom, the Ac arrays, lam[], the wave's row mask) and
// delassus_columns never reads its Shared&, so no LDS image is needed.  Not part of libopenroborl_hip.so; it includes the env kernels'
// header and instantiates no step or reset kernel.  A sibling of orr_probe.hip (the leaves these stages are built from).
//
//   extern "C" int orrp_<name>(const void* in, void* out, int n, int iters, void* stream)
//
// `in` / `out` are DEVICE pointers to n records of 4-byte words, one lane per record.  Whole waves only: n a multiple of 64, at least two
// blocks; record i sits in lane i & 63 of its wave, i.e. robot `sub` = (i >> 4) & 3 of the wave and `lane` = i & 15 of that robot (bank A:
// slot lane < 4 ? lane : lane + 12; bank B: slot lane, lanes 0..3 hold no row).  `iters` is a launch argument (0..32; anything else is
// refused), so no loop length depends on data.  Returns 0, -1 for bad arguments, or the hipError_t of the launch.
// The _a entry points run the <false> instantiations (no joint-limit bank), the _ab ones the <true> instantiations; both read the same
// record layout (the _a ones ignore the bank-B words).  Integer fields travel as float values, the row mask as its bit pattern.
//
// orrp_pgs_a / orrp_pgs_ab: pgs_sweeps alone.
//   in  (105): A: lam w jdi rhs cfm lo_c hi_c mu_e lam_n nrm_slot | B: the same ten | AcA[28] | AcB[28] | lam[28] | mask
//   out  (28): lam[28]
// orrp_delassus_pgs_a / orrp_delassus_pgs_ab: delassus_columns, then pgs_sweeps, as physics_substep runs them.
//   in   (75): A: active leg nrm_slot jl[3] rhs jdi lam cfm lo_c hi_c mu_e wa[6] wq[12] | B: the same 31 | ContactGeom (12) | mask
//              (rhs already multiplied by jdi, as row_response leaves it; w = cfm * lam is set here, as row_response does)
//   out (115): AcA[28] | AcB[28] | lam[28] before the sweeps | A.w B.w A.lam_n before the sweeps | lam[28] after them
#include "orr_env_kernels.h"

namespace {

constexpr int kPgsRow = 10, kPgsIn = 2 * kPgsRow + 3 * kMaxRows + 1, kPgsOut = kMaxRows;
constexpr int kDelRow = 31, kDelIn = 2 * kDelRow + 12 + 1, kDelOut = 4 * kMaxRows + 3;

__device__ __forceinline__ void clear_row(Row& R) {
  R.active = false; R.leg = 0; R.nrm_slot = -1; R.warm = -1;
#pragma unroll
  for (int k = 0; k < 6; k++) { R.Jb[k] = 0.0f; R.wa[k] = 0.0f; }
#pragma unroll
  for (int k = 0; k < 3; k++) R.jl[k] = 0.0f;
#pragma unroll
  for (int k = 0; k < 12; k++) R.wq[k] = 0.0f;
  R.rhs = 0.0f; R.jdi = 0.0f; R.lam = 0.0f; R.w = 0.0f; R.lam_n = 0.0f; R.cfm = 0.0f; R.lo_c = 0.0f; R.hi_c = 0.0f; R.mu_e = 0.0f;
}
__device__ __forceinline__ void load_pgs_row(const float* a, Row& R) {
  clear_row(R);
  R.lam = a[0]; R.w = a[1]; R.jdi = a[2]; R.rhs = a[3]; R.cfm = a[4]; R.lo_c = a[5]; R.hi_c = a[6]; R.mu_e = a[7]; R.lam_n = a[8];
  R.nrm_slot = (int)a[9];
}
__device__ __forceinline__ void load_delassus_row(const float* a, Row& R) {
  clear_row(R);
  R.active = a[0] != 0.0f; R.leg = (int)a[1]; R.nrm_slot = (int)a[2];
  R.jl[0] = a[3]; R.jl[1] = a[4]; R.jl[2] = a[5];
  R.rhs = a[6]; R.jdi = a[7]; R.lam = a[8]; R.cfm = a[9]; R.lo_c = a[10]; R.hi_c = a[11]; R.mu_e = a[12];
#pragma unroll
  for (int k = 0; k < 6; k++) R.wa[k] = a[13 + k];
#pragma unroll
  for (int k = 0; k < 12; k++) R.wq[k] = a[19 + k];
  R.w = R.cfm * R.lam;
}

// whole waves: no lane leaves before the stage ran (n is a multiple of 64: the entry point checked it)
template <bool HAS_B>
__global__ __launch_bounds__(64) void pgs_kernel(const float* __restrict__ in, float* __restrict__ out, int n, int iters) {
  if (((int)blockIdx.x + 1) * 64 > n) return;   // wave-uniform
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  const int sub = ((int)threadIdx.x >> 4) & 3, lane = (int)threadIdx.x & 15;
  const float* a = in + (size_t)i * kPgsIn;
  Row A, B;
  load_pgs_row(a, A);
  load_pgs_row(a + kPgsRow, B);
  float AcA[kMaxRows], AcB[kMaxRows], lam[kMaxRows];
#pragma unroll
  for (int r = 0; r < kMaxRows; r++) {
    AcA[r] = a[2 * kPgsRow + r]; AcB[r] = a[2 * kPgsRow + kMaxRows + r]; lam[r] = a[2 * kPgsRow + 2 * kMaxRows + r];
  }
  const unsigned int mask = (unsigned int)__builtin_amdgcn_readfirstlane(__float_as_int(a[kPgsIn - 1]));
  pgs_sweeps<HAS_B>(iters, mask, lane, sub, A, B, AcA, AcB, lam);
#pragma unroll
  for (int r = 0; r < kMaxRows; r++) out[(size_t)i * kPgsOut + r] = lam[r];
}

template <bool HAS_B>
__global__ __launch_bounds__(64) void delassus_pgs_kernel(const float* __restrict__ in, float* __restrict__ out, int n, int iters) {
  __shared__ Shared Sarr[kRPW];                  // never read (delassus_columns takes the reference and does not use it)
  if (((int)blockIdx.x + 1) * 64 > n) return;   // wave-uniform
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  const int sub = ((int)threadIdx.x >> 4) & 3, lane = (int)threadIdx.x & 15;
  const float* a = in + (size_t)i * kDelIn;
  float* o = out + (size_t)i * kDelOut;
  Row A, B;
  load_delassus_row(a, A);
  load_delassus_row(a + kDelRow, B);
  const float* g = a + 2 * kDelRow;
  const ContactGeom G = {g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11]};
  const unsigned int mask = (unsigned int)__builtin_amdgcn_readfirstlane(__float_as_int(a[kDelIn - 1]));
  float AcA[kMaxRows], AcB[kMaxRows], lam[kMaxRows];
#pragma unroll
  for (int r = 0; r < kMaxRows; r++) lam[r] = 0.0f;   // delassus_columns<false> leaves lam[4..15] unset
  delassus_columns<HAS_B>(Sarr[sub], mask, lane, sub, A, B, G, AcA, AcB, lam);
#pragma unroll
  for (int r = 0; r < kMaxRows; r++) { o[r] = AcA[r]; o[kMaxRows + r] = AcB[r]; o[2 * kMaxRows + r] = lam[r]; }
  o[3 * kMaxRows] = A.w; o[3 * kMaxRows + 1] = B.w; o[3 * kMaxRows + 2] = A.lam_n;
  pgs_sweeps<HAS_B>(iters, mask, lane, sub, A, B, AcA, AcB, lam);
#pragma unroll
  for (int r = 0; r < kMaxRows; r++) o[3 * kMaxRows + 3 + r] = lam[r];
}

template <typename K>
int launch(K kernel, const void* in, void* out, int n, int iters, void* stream) {
  if (n < 128 || n % 64 != 0 || !in || !out || iters < 0 || iters > 32) return -1;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(n / 64)), dim3(64), 0, (hipStream_t)stream, (const float*)in, (float*)out, n, iters);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int orrp_pgs_a(const void* in, void* out, int n, int iters, void* stream) { return launch(pgs_kernel<false>, in, out, n, iters, stream); }
extern "C" int orrp_pgs_ab(const void* in, void* out, int n, int iters, void* stream) { return launch(pgs_kernel<true>, in, out, n, iters, stream); }
extern "C" int orrp_delassus_pgs_a(const void* in, void* out, int n, int iters, void* stream) {
  return launch(delassus_pgs_kernel<false>, in, out, n, iters, stream);
}
extern "C" int orrp_delassus_pgs_ab(const void* in, void* out, int n, int iters, void* stream) {
  return launch(delassus_pgs_kernel<true>, in, out, n, iters, stream);
}
extern "C" int orrp_solver_record_words(int which) {   // 0..3: pgs in / out, delassus_pgs in / out (the loader checks its mirror)
  return which == 0 ? kPgsIn : which == 1 ? kPgsOut : which == 2 ? kDelIn : which == 3 ? kDelOut : -1;
}
