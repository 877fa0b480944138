// orr_kernels_shaping.hip -- the shaped reward (orr_shaped_reward, include/openroborl_hip.h): six penalty terms per robot from what the
// step just taken left behind (the action, the bound actuator / contact outputs, three integers of the state record), the reward less
// their weighted sum, and the running sums of both.  The thirteenth unit of the env kernels and, like orr_kernels_priv.hip, no variant of
// step or reset: a post-step gather of ~0.6 KB per robot, sized by the launch latency, compiled with the plain flags.
//
// Mapping: sixteen lanes per robot, four robots per wave, as in the env kernels; a workgroup is one wave.
//   loads   lane m < 12 fetches its motor's act_dev row; lanes 0..3 the legs' contact rows, 4..6 the action row, 7..12 the prev row,
//           13..15 the record's pieces that hold EP_STEP, LAST_EP_LEN and DONE_REASON (one 16-byte piece each); lanes 0..1 the two halves
//           of the episode row and of the totals row; every lane the robot's reward and done byte (one address each).  All in flight
//           together; only the table's pointers and weights come first (what the handle holds when the launch RUNS).
//   terms   the 12- and 4-element sums over the DPP row (row_sum16), in every lane; the action and prev words cross lanes through LDS
//   stores  behind every load (the staging hand-off waits for them): lanes 0..1 the halves of the three sum rows, lanes 2..7 the new prev
//           row, lane 8 the reward.  A padding lane group shadows robot 0 and stores nothing.  No atomics: the same inputs, the same bits.
#include "orr_env_kernels.h"

namespace {

constexpr int kPieceEpStep = ORR_OFF_EP_STEP / 4, kPieceLastLen = ORR_OFF_LAST_EP_LEN / 4, kPieceReason = ORR_OFF_DONE_REASON / 4;
constexpr int kRowQ = ORR_SHAPING_ROW / 4;                                       // 16-byte pieces of a sum row
constexpr int kFailBits = ORR_DONE_CONTACT_FALL | ORR_DONE_ROOT_POS | ORR_DONE_ROOT_ROT | ORR_DONE_NAN;
static_assert(kLanes == 16 && kRPW == 4, "one DPP row per robot");
static_assert(ORR_SHAPING_TERMS == 6 && ORR_SHAPING_ROW == 8 && kRowQ == 2, "a row is {p0..p5, shaped, 1}: two 16-byte pieces");
static_assert(sizeof(orr_reward_shaping) == 4 * (ORR_SHAPING_TERMS + 1), "six weights and the floor");
// the table's pointers are generic; the buffers behind them are global memory: say so, or every access is a flat one that also counts as an LDS access
typedef f4 __attribute__((address_space(1)))* gf4;
typedef const f4 __attribute__((address_space(1)))* gcf4;
static_assert(ORR_OFF_DONE_REASON < ORR_OFF_RING && ORR_OFF_EP_STEP < ORR_OFF_RING, "the integers sit in the record's head");

__global__ __launch_bounds__(64) void orr_shaped_reward_kernel(const DevTables* __restrict__ tab, const float* __restrict__ state, int n,
                                                               const float* __restrict__ actions, const float* reward_in,
                                                               const uint8_t* __restrict__ done, float* reward_out, float inv_nsub, float inv_dt) {
  __shared__ __attribute__((aligned(16))) f4 stage[kRPW][kLanes];   // per robot: the second load of every lane (contact | action | prev | integers)
  const int wtid = (int)threadIdx.x, sub = wtid / kLanes, lane = wtid % kLanes;
  const int robot_raw = (int)blockIdx.x * kRPW + sub;
  const bool in_range = robot_raw < n;
  const int robot = in_range ? robot_raw : 0;          // a padding lane group shadows robot 0 and stores nothing
  const f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  // ---- the table: what the handle has set and bound when the launch RUNS (a replayed graph follows the setter and a rebind) ----
  const gcf4 act4 = (gcf4)tab->act_out, contact4 = (gcf4)tab->contact_out;
  const gf4 shape4 = (gf4)tab->shape_out, ep4 = (gf4)tab->shape_ep, tot4 = (gf4)tab->shape_tot, prev4 = (gf4)tab->shape_prev;
  const orr_reward_shaping W = tab->shaping;
  // ---- loads: all in flight together ----
  const gcf4 rec4 = (gcf4)(state + (size_t)robot * ORR_STATE_STRIDE);
  // every lane issues every load, without a branch (a branch per load would put a wait in front of the next one): a lane that has no
  // piece to fetch reads piece 0 of its robot's record instead, and a select drops what it got
  const bool has_act = lane < 12 && act4 != nullptr, has_contact = lane < 4 && contact4 != nullptr;
  const gcf4 pa = has_act ? act4 + (size_t)robot * 12 + lane : rec4;
  gcf4 ps = rec4 + (lane == 13 ? kPieceEpStep : (lane == 14 ? kPieceLastLen : kPieceReason));
  if (lane < 13) ps = (gcf4)prev4 + (size_t)robot * 6 + (lane - 7);
  if (lane < 7) ps = (gcf4)actions + (size_t)robot * 3 + (lane - 4);
  if (lane < 4) ps = has_contact ? contact4 + (size_t)robot * 4 + lane : rec4;
  const gcf4 pe = lane < kRowQ ? (gcf4)ep4 + (size_t)robot * kRowQ + lane : rec4;
  const gcf4 pt = lane < kRowQ ? (gcf4)tot4 + (size_t)robot * kRowQ + lane : rec4;
  f4 A = *pa, second = *ps;
  const f4 ep_old = *pe, tot_old = *pt;
  const float r = reward_in[robot];
  const int done_byte = done[robot];
  // everything issued HERE and whole until here: one wait covers all of it.  (Left alone, the compiler sinks the two scalar loads behind
  // the sums and reuses the unread words of a row's registers for address arithmetic, which puts a wait between the loads.)
  asm volatile("" ::"v"(A), "v"(second), "v"(ep_old), "v"(tot_old), "v"(r), "v"(done_byte));
  const bool d = done_byte != 0;
  if (!has_act) A = zero;
  if (lane < 4 && !has_contact) second = zero;
  stage[sub][lane] = second;
  __syncthreads();
  // ---- the step's number within its episode and its done reason ----
  const float* sw = reinterpret_cast<const float*>(&stage[sub][0]);
  const int ep_step = __float_as_int(sw[4 * 13 + ORR_OFF_EP_STEP % 4]), last_len = __float_as_int(sw[4 * 14 + ORR_OFF_LAST_EP_LEN % 4]);
  const int reason = __float_as_int(sw[4 * 15 + ORR_OFF_DONE_REASON % 4]);
  const int n_step = d ? last_len : ep_step;
  const bool nan_step = (reason & ORR_DONE_NAN) != 0;
  // ---- the terms, in every lane ----
  const bool motor = lane < 12;
  const int j = motor ? lane : 0;
  const float a = sw[4 * 4 + j], a1 = sw[4 * 7 + j], a2 = sw[4 * 10 + j];
  const float d1 = a - a1, d2 = (a - 2.0f * a1) + a2;
  const float s_tau = row_sum16(motor ? A[2] : 0.0f);
  const float s_work = row_sum16(motor ? fabsf(A[3]) : 0.0f);
  const float s_rate = row_sum16(motor ? d1 * d1 : 0.0f);
  const float s_accel = row_sum16(motor ? d2 * d2 : 0.0f);
  const float s_peak = row_sum16(lane < 4 ? second[3] : 0.0f);
  const float p0 = nan_step ? 0.0f : s_tau * inv_nsub;
  const float p1 = nan_step ? 0.0f : s_work;
  const float p2 = nan_step || n_step < 2 ? 0.0f : s_rate;
  const float p3 = nan_step || n_step < 3 ? 0.0f : s_accel;
  const float p4 = nan_step ? 0.0f : s_peak * inv_dt;
  const float p5 = d && (reason & kFailBits) != 0 ? 1.0f : 0.0f;
  float pen = __builtin_fmaf(W.w[0], p0, 0.0f);
  pen = __builtin_fmaf(W.w[1], p1, pen);
  pen = __builtin_fmaf(W.w[2], p2, pen);
  pen = __builtin_fmaf(W.w[3], p3, pen);
  pen = __builtin_fmaf(W.w[4], p4, pen);
  pen = __builtin_fmaf(W.w[5], p5, pen);
  const float shaped = fmaxf(r - pen, W.floor);
  // ---- stores: behind every load of the wave ----
  if (!in_range) return;
  if (lane < kRowQ) {
    const f4 row = lane == 0 ? f4{p0, p1, p2, p3} : f4{p4, p5, shaped, 1.0f};
    const f4 ep_new = n_step <= 1 ? row : ep_old + row;
    const size_t at = (size_t)robot * kRowQ + lane;
    shape4[at] = row;
    ep4[at] = ep_new;
    if (d) tot4[at] = tot_old + ep_new;
  } else if (lane < 8) {
    prev4[(size_t)robot * 6 + (lane - 2)] = stage[sub][4 + (lane - 2)];    // {a, a1}: the staged pieces 4..9
  } else if (lane == 8) {
    reward_out[robot] = shaped;
  }
}

// the weights and the floor -> the device table, in stream order (orr_set_reward_shaping)
__global__ void orr_set_shaping_kernel(DevTables* tab, orr_reward_shaping s) { tab->shaping = s; }

}  // namespace

namespace orr {
hipError_t launch_shaped_reward(const DevTables* tab, const float* state, int n, const float* actions, const float* reward_in, const uint8_t* done,
                                float* reward_out, float inv_nsub, float inv_dt, hipStream_t stream) {
  hipLaunchKernelGGL(orr_shaped_reward_kernel, dim3((unsigned)((n + kRPW - 1) / kRPW)), dim3(64), 0, stream, tab, state, n, actions, reward_in, done,
                     reward_out, inv_nsub, inv_dt);
  return hipGetLastError();
}
hipError_t launch_set_shaping(DevTables* tab, const orr_reward_shaping& s, hipStream_t stream) {
  hipLaunchKernelGGL(orr_set_shaping_kernel, dim3(1), dim3(1), 0, stream, tab, s);
  return hipGetLastError();
}
}  // namespace orr
