// orr_kernels_priv.hip -- the privileged observation (orr_privileged_obs, include/openroborl_hip.h): one row of ORR_PRIV_DIM words per
// robot, gathered from the state record's head and the handle's bound contact / push outputs.  The twelfth unit of the env kernels and
// the only one with the plain flags: the kernel is a gather of ~0.4 KB per robot, sized by the launch latency, and shares no code with
// the step and reset kernels beyond the quaternion helpers of orr_device.h.
//
// Mapping: sixteen lanes per robot, four robots per wave, as in the env kernels; a workgroup is one wave.
//   loads   lane l < 13 fetches one 16-byte piece of the record's head (of its 77 pieces only the 13 that hold a word of the row:
//           pieces 0..3 = POS QUAT LINVEL ANGVEL, kParam0.. = STRENGTH .. INERTIA_RATIO, kInt0.. = EP_STEP MAX_EP_STEPS ROBOT_TYPE);
//           lanes 0..3 also fetch the leg's contact row and lanes 4..5 the two halves of the push row (one 16-byte piece each); every lane
//           reads the robot's done byte (one address).  All in flight together; only INIT_QUAT of the robot's type is a dependent load (it needs ROBOT_TYPE).
//   row     lane l forms words l, 16 + l and 32 + l from the staged pieces (LDS), every lane its own copy of the rotation
//   stores  the wave's four rows are 192 consecutive floats: lanes 0..47 store one 16-byte piece each (768 contiguous bytes)
#include "orr_env_kernels.h"

namespace {

constexpr int kParam0 = ORR_OFF_STRENGTH / 4;                          // first and
constexpr int kParamN = ORR_OFFEND_INERTIA_RATIO / 4 - kParam0 + 1;    //   number of the pieces that hold STRENGTH .. INERTIA_RATIO
constexpr int kInt0 = ORR_OFF_EP_STEP / 4;
constexpr int kIntN = ORR_OFF_ROBOT_TYPE / 4 - kInt0 + 1;
constexpr int kPieces = 4 + kParamN + kIntN;
static_assert(ORR_OFFEND_ANGVEL < 16 && ORR_OFF_POS == 0, "POS QUAT LINVEL ANGVEL sit in the first four pieces");
static_assert(ORR_OFF_INERTIA_RATIO + 1 == ORR_OFFEND_INERTIA_RATIO && ORR_OFF_STRENGTH + 12 == ORR_OFF_LATENCY && ORR_OFF_LATENCY + 1 == ORR_OFF_FOOT_MU &&
              ORR_OFF_FOOT_MU + 1 == ORR_OFF_KNEE_FRICTION && ORR_OFF_KNEE_FRICTION + 4 == ORR_OFF_MASS_RATIO && ORR_OFF_MASS_RATIO + 2 == ORR_OFF_INERTIA_RATIO,
              "words 10..31 of the row are one run of the record (STRENGTH .. INERTIA_RATIO)");
static_assert(ORR_OFF_EP_STEP < ORR_OFF_MAX_EP_STEPS && ORR_OFF_MAX_EP_STEPS < ORR_OFF_ROBOT_TYPE && ORR_OFF_ROBOT_TYPE < ORR_OFF_RING, "the integers' pieces");
static_assert(kPieces <= kLanes && kLanes == 16 && kRPW == 4, "one piece of the head per lane");
static_assert(ORR_PRIV_DIM == 3 * kLanes && ORR_PRIV_DIM % 4 == 0 && kRPW * ORR_PRIV_DIM / 4 <= 64, "three words per lane; the wave's rows in 16-byte pieces");
static_assert(ORR_PUSH_ROW == 8, "the push row is two 16-byte pieces");

struct PrivStage {            // per robot, LDS
  f4 head[kLanes];            // the fetched pieces: [0..3] words 0..15, [4 ..] STRENGTH .., [4 + kParamN ..] the integers
  f4 contact[4];              // per leg: the contact row (zeros where masked)
  f4 push[2];                 // the push row (zeros where masked)
  float row[ORR_PRIV_DIM];
};

__device__ __forceinline__ float head_word(const PrivStage& T, int first_piece, int slot0, int off) {   // word `off` of the record, from the run of pieces that starts at slot0
  const float* w = reinterpret_cast<const float*>(&T.head[slot0]);
  return w[off - 4 * first_piece];
}

__global__ __launch_bounds__(64) void orr_privileged_obs_kernel(const DevTables* __restrict__ tab, const float* __restrict__ state, int n,
                                                                const uint8_t* __restrict__ done, float* __restrict__ priv, float lat_div, float step_dt) {
  __shared__ __attribute__((aligned(16))) PrivStage Tarr[kRPW];
  const int wtid = (int)threadIdx.x, sub = wtid / kLanes, lane = wtid % kLanes;
  const int robot_raw = (int)blockIdx.x * kRPW + sub;
  const bool in_range = robot_raw < n;
  const int robot = in_range ? robot_raw : 0;          // a padding lane group shadows robot 0 and stores nothing
  PrivStage& T = Tarr[sub];
  const f4* rec4 = reinterpret_cast<const f4*>(state + (size_t)robot * ORR_STATE_STRIDE);
  const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  // ---- loads: everything but INIT_QUAT in flight together ----
  const int piece = lane < 4 ? lane : (lane < 4 + kParamN ? kParam0 + (lane - 4) : (lane < kPieces ? kInt0 + (lane - 4 - kParamN) : 0));
  const f4 hp = rec4[piece];
  const float* contact_out = tab->contact_out;         // what the handle has bound when the launch RUNS (a replayed graph follows a rebind)
  const float* push_out = tab->push_out;
  f4 extra = zero;
  if (done) {                                          // NULL: after a reset the buffers hold no step of the current episode
    if (lane < 4 && contact_out) extra = reinterpret_cast<const f4*>(contact_out)[(size_t)robot * 4 + lane];
    if (lane >= 4 && lane < 6 && push_out) extra = reinterpret_cast<const f4*>(push_out)[(size_t)robot * 2 + (lane - 4)];
  }
  const bool ended = done ? done[robot] != 0 : true;   // the buffers still describe the episode that ended
  if (ended) extra = zero;
  T.head[lane] = hp;
  if (lane < 4) T.contact[lane] = extra;
  else if (lane < 6) T.push[lane - 4] = extra;
  __syncthreads();
  // ---- the rotation: rel = QUAT (x) INIT_QUAT^-1 as base_rotation forms it, R by the standard formula (rel as it is) ----
  const float* h0 = reinterpret_cast<const float*>(&T.head[0]);
  const int type = __float_as_int(head_word(T, kInt0, 4 + kParamN, ORR_OFF_ROBOT_TYPE));
  const int type_ok = (unsigned)type < (unsigned)ORR_MAX_ROBOT_TYPES ? type : 0;   // a record that was never initialised must not index past the table
  const f4 iq4 = *reinterpret_cast<const f4*>(tab->model[type_ok].hot.init_quat);
  static_assert(offsetof(ModelHot, init_quat) % 16 == 0, "one 16-byte load");
  const float iq[4] = {iq4[0], iq4[1], iq4[2], iq4[3]};
  float qi[4], rel[4];
  qinv(iq, qi);
  qmul(h0 + ORR_OFF_QUAT, qi, rel);
  const float x = rel[0], y = rel[1], z = rel[2], w = rel[3];
  const float R[9] = {1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - z * w), 2.0f * (x * z + y * w),
                      2.0f * (x * y + z * w), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - x * w),
                      2.0f * (x * z - y * w), 2.0f * (y * z + x * w), 1.0f - 2.0f * (x * x + y * y)};
  const float down[3] = {0.0f, 0.0f, -1.0f};
  float lin[3], ang[3], grav[3];
  mtv3(R, h0 + ORR_OFF_LINVEL, lin);
  mtv3(R, h0 + ORR_OFF_ANGVEL, ang);
  mtv3(R, down, grav);
  // ---- word lane (0..15): the rotated vectors, the height, STRENGTH[0..5] ----
  float a;
  if (lane < 3) a = pick4(lane, lin[0], lin[1], lin[2], 0.0f);
  else if (lane < 6) a = pick4(lane - 3, ang[0], ang[1], ang[2], 0.0f);
  else if (lane < 9) a = pick4(lane - 6, grav[0], grav[1], grav[2], 0.0f);
  else if (lane == 9) a = h0[ORR_OFF_POS + 2];
  else a = head_word(T, kParam0, 4, ORR_OFF_STRENGTH + (lane - 10));
  // ---- word 16 + lane (16..31): STRENGTH[6..11], LATENCY, FOOT_MU, KNEE_FRICTION, MASS_RATIO, INERTIA_RATIO: one run of the record ----
  float b = head_word(T, kParam0, 4, ORR_OFF_STRENGTH + 6 + lane);
  if (lane == 22 - 16) b = b / lat_div;
  else if (lane >= 24 - 16 && lane < 28 - 16) b = b * 20.0f;
  // ---- word 32 + lane (32..47): contact flags, mean normal forces, the push, the episode's progress, 0 ----
  float c = 0.0f;
  if (lane < 8) {
    const float nsum = T.contact[lane & 3][0];
    c = lane < 4 ? (nsum > 0.0f ? 1.0f : 0.0f) : nsum / step_dt / 100.0f;
  } else if (lane < 14) {
    c = reinterpret_cast<const float*>(T.push)[lane - 8];
  } else if (lane == 14) {
    const int ep = __float_as_int(head_word(T, kInt0, 4 + kParamN, ORR_OFF_EP_STEP)), mx = __float_as_int(head_word(T, kInt0, 4 + kParamN, ORR_OFF_MAX_EP_STEPS));
    c = (float)ep / (float)(mx > 1 ? mx : 1);
  }
  T.row[lane] = a;
  T.row[kLanes + lane] = b;
  T.row[2 * kLanes + lane] = c;
  __syncthreads();
  // ---- stores: the wave's rows as consecutive 16-byte pieces (rows of robots beyond n are not written) ----
  constexpr int kRowQ = ORR_PRIV_DIM / 4;
  if (wtid < kRPW * kRowQ) {
    const int r = wtid / kRowQ, q = wtid - r * kRowQ;
    if ((int)blockIdx.x * kRPW + r < n)
      reinterpret_cast<f4*>(priv)[((size_t)blockIdx.x * kRPW + r) * kRowQ + q] = reinterpret_cast<const f4*>(Tarr[r].row)[q];
  }
}

}  // namespace

namespace orr {
hipError_t launch_privileged_obs(const DevTables* tab, const float* state, int n, const uint8_t* done, float* priv, float lat_div, float step_dt,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(orr_privileged_obs_kernel, dim3((unsigned)((n + kRPW - 1) / kRPW)), dim3(64), 0, stream, tab, state, n, done, priv, lat_div, step_dt);
  return hipGetLastError();
}
}  // namespace orr
