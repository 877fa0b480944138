// orr_env_kernels.h -- the two env kernels (orr_reset_kernel, orr_step_kernel) and their launchers, as templates.
//
// Included by the eleven translation units of the env kernels; each unit instantiates its own variants and nothing else (why there are
// several: DESIGN.md section 3).  orr_kernels.hip: the default kernels + the C-ABI, instruction-level-parallelism scheduler (one wave per
// SIMD, ~300 registers, nothing to hide latency but the wave's own independent instructions).  orr_kernels_w2.hip: the
// two-waves-per-SIMD step kernel, its own flags.  orr_kernels_anchor.hip: the friction-anchor variants.  orr_kernels_multiclip.hip:
// the clip-set variants.  orr_kernels_noise.hip: the task-noise variants (clip sets + perturbed initial states + target-heading noise).
// orr_kernels_terms.hip: the noise variant of the step that also writes the per-term reward outputs (orr_bind_reward_terms).
// orr_kernels_contacts.hip: the variants that also sum the sub-steps' foot contact impulses (orr_bind_contact_outputs).
// orr_kernels_actuator.hip: the variants that clip the motor torques and keep per-motor torque / work accumulators (orr_set_torque_limits,
// orr_bind_actuator_outputs).  orr_kernels_sensor.hip: the variants whose sensor readings carry Gaussian noise (orr_set_sensor_noise).
// orr_kernels_randomizer.hip: the variants whose resets run the table-driven randomiser (orr_set_randomizer, orr_bind_randomizer_params).
// orr_kernels_push.hip: the env step that kicks the robot's base twist (orr_set_push, orr_bind_push_outputs).
// (A twelfth unit, orr_kernels_priv.hip, includes this header for the record's layout and the device table only: it holds the kernel of
// orr_privileged_obs, no variant of step or reset, and is compiled with the plain flags.  A thirteenth, orr_kernels_shaping.hip, does the
// same for the kernel of orr_shaped_reward.)
// An instantiation compiled next to the default ones moves the default kernels' code (round 5: +6 instructions
// per sub-step, +0.7 % run time with the anchor variants alongside), so the main unit sees the other units' launchers as `extern
// template` only (bottom of this file).
// Device code by phase: orr_device.h (LDS image, math, DPP helpers), orr_robot_io.h (record load / store, latency ring),
// orr_physics.h (one physics sub-step), orr_task.h (motion clips, reward, observation, reset).
// A unit may set two properties before the include: ORR_TU_STEP_W2 + ORR_PARITY (orr_kernels_w2.hip; orr_physics.h, orr_device.h)
// and ORR_TU_MAIN (orr_kernels.hip: the unit that holds the development timers' and counters' globals).
#pragma once
// The phase timers' build also records the per-wave timeline.  Decided HERE, in front of the line that keeps the timers to the main
// unit: KParams (which carries the timeline's buffer) is a by-value kernel argument built in the main unit and consumed by the other
// units' launchers, so all four have to see the same struct.
#if defined(ORR_PHASE_TIMERS) && !defined(ORR_WAVE_TIMELINE)
#define ORR_WAVE_TIMELINE 1
#endif
#ifndef ORR_TU_MAIN
#undef ORR_PHASE_TIMERS      // the development timers live in the main translation unit only
#endif
#include <hip/hip_runtime.h>
#include <type_traits>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// The constraint rows need A0^-1 (Jb - T_L jl): every row lane solves with the Cholesky factor of A0, which stays in registers (15 entries + 6 reciprocal pivots, Chol6Pk) from
// the leg dynamics on (-54 instructions per sub-step there: no unit-column solve, no A0^-1 through LDS; +15 per bank in the row
// response).  4096 robots 0.2338 -> 0.2295 ms; the two-wave unit (256 registers, spilling) is neutral (8192 robots 0.3265 vs 0.3255 ms)
// and takes it too, so that both variants of the kernel keep giving the same bits.
#include "orr_device.h"

// Development aid (tools/phase_cycles.py): -DORR_PHASE_TIMERS makes lane 0 of one wave accumulate shader-clock cycles
// per phase (Shared::pt_acc) and add them to g_phase_cycles at the end of the launch.  It implies -DORR_WAVE_TIMELINE (top of this file).
#ifdef ORR_PHASE_TIMERS
__device__ long long g_phase_cycles[orr::kPhaseSlots];   // 0..15: phases of the step, 16..23: stages of reset_robot_state, 24..: finer marks inside the reset
__device__ long long g_wave_phases[2048 * 40];   // per wave of the last launch: its own phase totals (tools/wave_phases.py)
#define PT_INIT() do { if (threadIdx.x == 0) { for (int i_ = 0; i_ < orr::kPhaseSlots; i_++) S.pt_acc[i_] = 0; S.pt_last = clock64(); } } while (0)
#define PT(k) do { if (threadIdx.x == 0) { const long long t_ = clock64(); S.pt_acc[k] += t_ - S.pt_last; S.pt_last = clock64(); } } while (0)
#define PT_FLUSH() do { if (threadIdx.x == 0 && blockIdx.x == gridDim.x / 2) for (int i_ = 0; i_ < orr::kPhaseSlots; i_++) atomicAdd((unsigned long long*)&g_phase_cycles[i_], (unsigned long long)S.pt_acc[i_]); \
                        if (threadIdx.x == 0 && blockIdx.x < 2048) for (int i_ = 0; i_ < orr::kPhaseSlots; i_++) g_wave_phases[blockIdx.x * 40 + i_] = S.pt_acc[i_]; } while (0)
#else
#define PT_INIT()
#define PT(k)
#define PT_FLUSH()
#endif

// Development aid (tools/wave_times.py, and the phase timers' tools): -DORR_WAVE_TIMELINE makes every wave of the step kernel - EVERY
// variant, product code otherwise - record when it started and ended (100 MHz realtime counter), its shader cycles, which of its robots
// finished an episode and the hardware slot it ran on (nothing else is instrumented: two s_memrealtime / s_memtime pairs and one
// 32-byte store per wave, into KParams::wave_times once orr_debug_wave_times has allocated it, for the waves it has room for)
#ifdef ORR_WAVE_TIMELINE
#define WT_INIT() const long long wt_r0 = wall_clock64(), wt_c0 = clock64()
#define WT_STORE(flag) do { if (threadIdx.x == 0 && wave_id < P.wave_times_cap) { long long* w_ = P.wave_times + 4 * (size_t)wave_id; w_[0] = wt_r0; w_[1] = wall_clock64(); w_[2] = clock64() - wt_c0; \
    w_[3] = ((flag) & 0xFF) | ((long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 8) | ((long long)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xF) << 40); } } while (0)   /* bits 8..39: HW_REG_HW_ID (wave, simd, cu, sh, se), 40..43: HW_REG_XCC_ID */
#else
#define WT_INIT()
#define WT_STORE(flag)
#endif

// Development aid (tools/dual_contact.py): -DORR_COUNT_DUAL_CONTACT counts, per leg and sub-step, how often the toe sphere and the shank
// sphere of a lower leg are within the contact margin / penetrating at the same time (the engine makes ONE contact point per leg, Bullet
// one per touching shape: DESIGN.md section 9).  One-wave kernel only.
#if defined(ORR_COUNT_DUAL_CONTACT) && defined(ORR_TU_MAIN)
__device__ unsigned long long g_dual_contact[8];
// (called from row_setup_bank_a in every lane of the wave: the first ACTIVE lane adds the wave's count)
#define ORR_DUAL_COUNT(k, cond) do { const unsigned long long b_ = __ballot(cond), act_ = __ballot(1); \
    if (b_ && (int)(threadIdx.x & 63u) == __ffsll((long long)act_) - 1) atomicAdd(&g_dual_contact[k], (unsigned long long)__popcll(b_)); } while (0)
#else
#define ORR_DUAL_COUNT(k, cond)
#endif

using namespace orr;

#define O(name) ORR_OFF_##name

#include "orr_robot_io.h"
#include "orr_physics.h"
#include "orr_task.h"

// ================================================================================================
// kernels
// ================================================================================================
// lane group bookkeeping shared by the kernels: `sub` = which robot of this wave, `lane` = lane within the robot
// (a workgroup is one wave: an independent quad of robots)
#define ORR_PROLOGUE()                                                                   \
  __shared__ Shared Sarr[kRPW];                                                          \
  const int wtid = (int)threadIdx.x;                                                     \
  const int wave_id = (int)blockIdx.x;                                                   \
  const int sub = wtid / kLanes, lane = wtid % kLanes;                                   \
  Shared& S = Sarr[sub];                                                                 \
  float* obs = S.ph.end.obs;                                                             \
  const int robot_raw = wave_id * kRPW + sub;                                            \
  const bool in_range = robot_raw < P.cfg.num_robots;                                    \
  const int robot = in_range ? robot_raw : 0; /* a padding lane group shadows robot 0 and never stores */ \
  float* rec = P.state + (size_t)robot * ORR_STATE_STRIDE

// CLIPS: the multi-clip variant (orr_kernels_multiclip.hip): every reset draws the robot's clip from its type's clip set
// NOISE: the noise variant (orr_kernels_noise.hip, with CLIPS): perturbed initial states and target-heading noise (orr_set_task_noise)
template <bool CLIPS = false, bool NOISE = false>
__global__ __launch_bounds__(64) void orr_reset_kernel(KParams P, const uint8_t* mask, float* obs_out, const float* uniforms) {
  ORR_PROLOGUE();
  const bool valid = in_range && !(mask && !mask[robot]);
  load_robot(P, rec, S, lane);
  const long long total = P.counters[ORR_CNT_TOTAL_STEP_COUNT];
  const ResetConst RC = load_reset_const(P, S, lane);
  float clip_change = 0.0f;
  const uint32_t ep = reset_robot_state<CLIPS, NOISE>(P, S, lane, total, RC, &clip_change, uniforms ? uniforms + (size_t)robot * 28 : nullptr);
  build_obs<NOISE>(P, rec, S, lane, obs, ep, 0u);
  WSYNC();
  store_reset_extras<CLIPS>(rec, S, lane, valid, clip_change);
  store_robot(rec, S, lane, valid);
  // a new episode: no cached contact points (ANCHOR, ANCHOR_VALID: 28 words behind the ring).  Unconditional: friction anchors may be switched
  // on (orr_set_model) after this reset, and a caller-bound record need not have been zeroed
  if (valid)
    for (int i = lane; i < ORR_OFFEND_ANCHOR_VALID - ORR_OFF_ANCHOR + 1; i += kLanes) rec[O(ANCHOR) + i] = 0.0f;
  if (obs_out && valid)
    for (int i = lane; i < ORR_OBS_DIM; i += kLanes) obs_out[(size_t)robot * ORR_OBS_DIM + i] = obs[i];
}

// The reset of the sensor variants (orr_kernels_sensor.hip; orr_set_sensor_noise): orr_reset_kernel<CLIPS, true> with noisy sensor
// histories - three separate readings - and a noisy heading of the target observation.  A kernel of its own rather than a third
// parameter of orr_reset_kernel: the names of that kernel's instantiations stay exactly as they are
template <bool CLIPS = true>
__global__ __launch_bounds__(64) void orr_sensor_reset_kernel(KParams P, const uint8_t* mask, float* obs_out, const float* uniforms) {
  ORR_PROLOGUE();
  const bool valid = in_range && !(mask && !mask[robot]);
  load_robot(P, rec, S, lane);
  const long long total = P.counters[ORR_CNT_TOTAL_STEP_COUNT];
  const ResetConst RC = load_reset_const(P, S, lane);
  const SensorNoise SN = load_sensor_noise(P);
  float clip_change = 0.0f;
  const uint32_t ep = reset_robot_state<CLIPS, true, true>(P, S, lane, total, RC, &clip_change, uniforms ? uniforms + (size_t)robot * 28 : nullptr, SN);
  build_obs<true, true>(P, rec, S, lane, obs, ep, 0u, SN);
  WSYNC();
  store_reset_extras<CLIPS>(rec, S, lane, valid, clip_change);
  store_robot(rec, S, lane, valid);
  if (valid)      // a new episode: no cached contact points (as orr_reset_kernel)
    for (int i = lane; i < ORR_OFFEND_ANCHOR_VALID - ORR_OFF_ANCHOR + 1; i += kLanes) rec[O(ANCHOR) + i] = 0.0f;
  if (obs_out && valid)
    for (int i = lane; i < ORR_OBS_DIM; i += kLanes) obs_out[(size_t)robot * ORR_OBS_DIM + i] = obs[i];
}

// The reset of the randomiser variants (orr_kernels_randomizer.hip; orr_set_randomizer, orr_bind_randomizer_params):
// orr_sensor_reset_kernel with the table-driven stage 4b and the params row.  Suspended, the row's load is issued inside
// reset_robot_state with its first loads; otherwise the new row is stored here, with the record.  A kernel of its own for the same
// reason as orr_sensor_reset_kernel
template <bool CLIPS = true>
__global__ __launch_bounds__(64) void orr_randomizer_reset_kernel(KParams P, const uint8_t* mask, float* obs_out, const float* uniforms) {
  ORR_PROLOGUE();
  const bool valid = in_range && !(mask && !mask[robot]);
  load_robot(P, rec, S, lane);
  const long long total = P.counters[ORR_CNT_TOTAL_STEP_COUNT];
  const ResetConst RC = load_reset_const(P, S, lane);
  const SensorNoise SN = load_sensor_noise(P);
  RandRow RR = load_rand_row(P, robot);
  float clip_change = 0.0f;
  const uint32_t ep = reset_robot_state<CLIPS, true, true, true>(P, S, lane, total, RC, &clip_change, uniforms ? uniforms + (size_t)robot * 28 : nullptr, SN, &RR);
  build_obs<true, true>(P, rec, S, lane, obs, ep, 0u, SN);
  WSYNC();
  store_reset_extras<CLIPS>(rec, S, lane, valid, clip_change);
  store_rand_row(P, RR, lane, valid);
  store_robot(rec, S, lane, valid);
  if (valid)      // a new episode: no cached contact points (as orr_reset_kernel)
    for (int i = lane; i < ORR_OFFEND_ANCHOR_VALID - ORR_OFF_ANCHOR + 1; i += kLanes) rec[O(ANCHOR) + i] = 0.0f;
  if (obs_out && valid)
    for (int i = lane; i < ORR_OBS_DIM; i += kLanes) obs_out[(size_t)robot * ORR_OBS_DIM + i] = obs[i];
}

// mode 0: full env step.  mode 1 (debug / parity of row C): nsub physics sub-steps with the given
// motor torques (actions = torques), no robot or task logic.  mode 2 (parity of everything BUT row C): a full env step in
// which the physics sub-step is replaced by the recorded states of ReplayArgs, the end-effector reward reads recorded link
// positions and the fall flag is given -- the device-side counterpart of the oracle's replay mode, fed with the fixtures that the
// reference's own Python produced (tests/test_gpu_golden_task.py).
// WPE = waves per SIMD the kernel is compiled for.  WPE 1: up to 512 VGPRs (~300 used), one wave on each of the 1024 SIMDs = 4096 robots
// resident at once: the best a batch of <= 4096 robots can do.  WPE 2 (<= 256 VGPRs, 28 of them spilled, one scratch access inside the sub-step loop; LDS 19.3 KB per wave, so
// eight waves fit a CU): for larger batches.  A lone wave issues one vector instruction per ~5 cycles, the SIMD can take one per 2:
// two co-resident waves of this kernel take 1.12x as long as one alone (tools/wave_pairing.py), i.e. 1.8x the throughput per SIMD,
// where the WPE-1 kernel would run the second thousand waves after the first.  orr_step picks the variant from the batch size and the
// device's CU count (ORR_STEP_WAVES_PER_EU = 1 | 2 overrides, for measurements).
// (min, max) waves per SIMD are pinned to the same value: with a higher maximum this LLVM's iterative-ilp scheduler tries
// occupancy-improving reschedules once the kernel fits 256 VGPRs and then crashes in the register allocator.
#ifndef ORR_WAVES_PER_EU
#define ORR_WAVES_PER_EU 1   // development builds (-DORR_WAVES_PER_EU=2) force every instantiation to that occupancy
#endif
// ANCHOR (ABI v5): the variant for robot types with orr_model::friction_anchor - Bullet's cached toe contact points (orr_physics.h:
// AnchorState).  Same source; its own instantiations (one wave per SIMD whatever the batch size: an optional physics feature, not the
// measured path), so that the default kernels carry nothing of it.
// CLIPS: the multi-clip variant (orr_kernels_multiclip.hip, one wave per SIMD whatever the batch size): the auto-reset draws the new
// episode's clip from the robot type's clip set (reset_robot_state<true>), the episode log also records the clip of the ending episode, and
// a robot whose motion time has reached the record's CLIP_CHANGE_TIME switches to a newly drawn clip mid-episode (orr_set_clip_switch)
// NOISE: the noise variant (orr_kernels_noise.hip; instantiated with CLIPS only - a superset: a type without a clip set keeps its CLIP_ID -
// and one wave per SIMD whatever the batch size): the auto-reset may start the episode on a perturbed state and every target
// observation is expressed in a noisy heading (orr_set_task_noise; reset_robot_state<.., true>, target_obs<true>).  Both sit outside the
// sub-step loop.  LAST parameter: the mangled names of the other variants keep their prefixes (tools/isa_stats.py)
// TERMS = MODE & kModeTerms (orr_kernels_terms.hip; instantiated with CLIPS and NOISE only - a superset - and one wave per SIMD whatever the
// batch size): lanes 0..4 of a robot also store the five unweighted terms of the step's reward, keep their running sums over the episode
// in a caller-owned buffer and add the sums to the episode-log row (orr_bind_reward_terms).  All of it outside the sub-step loop.  A bit
// of MODE, not a sixth parameter: the names above stay as they are
// CONTACTS = MODE & kModeContacts (orr_kernels_contacts.hip; the env step on top of CLIPS and NOISE, with and without TERMS, and the debug
// physics; one wave per SIMD whatever the batch size): after every sub-step lanes 0..11 of a robot read their own word of the record's
// LAMBDA (slot 3 leg + d: the sub-step's normal and two friction impulses of a leg, 0 for an open contact) back from the LDS image and
// keep a running sum and a running maximum in registers: one LDS read, an add and a max per sub-step, nothing inside physics_substep.
// The row of the episode's totals is loaded with the reference frames, the stores come at the step's end, the log row goes where
// term_log's goes (orr_bind_contact_outputs)
// ACT = MODE & kModeActuator (orr_kernels_actuator.hip; the env step on top of CLIPS, NOISE, TERMS and CONTACTS and the parity replay on top
// of CLIPS, NOISE and TERMS - supersets: the loads and stores of the reward-terms and contact buffers are skipped where that binding's
// pointer is null - one wave per SIMD whatever the batch size): lane = motor clamps the sub-step's strength-scaled PD torque to +-the
// limit of its motor (DevTables::torque_limit, +inf = none: a select, so that the torque's bits pass) and keeps, in registers over the
// sub-steps, sum tau, max |tau|, sum tau^2 and sum tau qd of the motor-convention torque and the joint rate after the sub-step; the
// sub-step's torque stays in a register across physics_substep.  Nothing inside physics_substep.  The row of the episode's totals is
// loaded with the reference frames, the stores come at the step's end (one 16-byte store per motor lane), the log row goes where
// term_log's goes (orr_set_torque_limits, orr_bind_actuator_outputs)
// SENS = MODE & kModeSensor (orr_kernels_sensor.hip; on top of the two actuator variants - supersets - one wave per SIMD whatever the batch
// size): Minitaur._observation_noise_stdev (minitaur.py:370-375).  Lane = motor: every sub-step's +-max_angle_change clip reads a noisy
// motor angle, and so does the interpolation's start value while the episode has no filtered action yet, each with its own normal of
// the sub-step (one Philox block per motor and two sub-steps, the second pair of words kept in registers over the odd sub-step); the PD
// law keeps the true angle and rate.  Outside physics_substep, and skipped wave-uniformly while motor_angle_std is 0 (one setting per
// handle).  The filter history's initial value, the sensor histories' readings and the rpy that the target observation's heading is
// formed from are noisy too (sensors_push_noisy, target_obs<.., true>, reset_robot_state<.., true>): draw rule in
// include/openroborl_hip.h, orr_set_sensor_noise
// RAND = MODE & kModeRandomizer (orr_kernels_randomizer.hip; on top of the two sensor variants - supersets - one wave per SIMD whatever
// the batch size): the inline auto-reset runs the table-driven randomiser (reset_robot_state<.., RAND>; orr_set_randomizer) and writes
// or, suspended, applies the robot's row of the params buffer (orr_bind_randomizer_params).  Nothing in front of the episode's end: the
// buffer's address and the suspend switch are read at the start (scalars), the row's store comes with the record's
// PUSH = MODE & kModePush (orr_kernels_push.hip; the env step on top of the randomiser variant - a superset - one wave per SIMD whatever
// the batch size): a velocity kick of the base twist at the start of the step (orr_set_push), two Philox blocks and one sine / cosine per
// robot and step, on the LDS image ahead of the WSYNC that precedes load_own_coord.  Nothing inside the sub-step loop.  The settings are
// read at the start (scalars), the old count of the outputs row (orr_bind_push_outputs) with them, the row is stored at the step's end
template <int MODE, int WPE = ORR_WAVES_PER_EU, bool ANCHOR = false, bool CLIPS = false, bool NOISE = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void orr_step_kernel(KParams P, const float* actions, float* obs_out, float* reward_out,
                                                      uint8_t* done_out, int nsub, ReplayArgs RP) {
  constexpr bool TERMS = (MODE & kModeTerms) != 0;
  static_assert(!TERMS || (MODE & 3) != 1, "the debug physics computes no reward");
  constexpr bool CONTACTS = (MODE & kModeContacts) != 0;
  static_assert(!CONTACTS || (MODE & 3) != 2, "the parity replay replaces the physics by recorded states: it has no impulses");
  constexpr bool ACT = (MODE & kModeActuator) != 0;
  static_assert(!ACT || (MODE & 3) != 1, "the debug physics takes its torques as given");
  static_assert(!ACT || TERMS, "the actuator variants are supersets: instantiated with the reward terms only");
  constexpr bool SENS = (MODE & kModeSensor) != 0;
  static_assert(!SENS || (ACT && NOISE), "the sensor variants are supersets: instantiated on top of the actuator variants only");
  constexpr bool RAND = (MODE & kModeRandomizer) != 0;
  static_assert(!RAND || SENS, "the randomiser variants are supersets: instantiated on top of the sensor variants only");
  constexpr bool PUSH = (MODE & kModePush) != 0;
  static_assert(!PUSH || RAND, "the push variant is a superset: instantiated on top of the randomiser variant only");
  static_assert(!PUSH || (MODE & 3) == 0, "the parity replay replaces the physics by recorded states, the debug physics has no env step: neither is pushed");
  ORR_PROLOGUE();
  const bool valid = in_range;
  const orr_config& c = P.cfg;
  PT_INIT();
  WT_INIT();
  // curriculum counter as of the start of the launch (the last wave of the previous launch folded that launch's episodes in):
  // read here, far ahead of its only use (the time limit of an episode that starts in this launch)
  const long long total_snapshot = P.counters[ORR_CNT_TOTAL_STEP_COUNT];
  load_robot(P, rec, S, lane);
  // ACT: which of the three bindings this superset serves (wave-uniform); the other variants are instantiated for what is bound
  bool terms_bound = true, contacts_bound = true, act_bound = false;
  if constexpr (ACT) {
    terms_bound = P.tab->terms != nullptr;
    contacts_bound = P.tab->contact_out != nullptr;
    act_bound = P.tab->act_out != nullptr;
  }
  RandRow RR;   // RAND: the robot's row of the params buffer (wave-uniform address and switch)
  if constexpr (RAND) RR = load_rand_row(P, robot);
  // PUSH: the handle's settings (scalars) and the old count of kicks in the robot's row of the outputs (word 7; a padding lane group
  // shadows robot 0's and never stores): read here, first and last used at the kick below - nothing of PS lives across the sub-step
  // loop (the step end reads the buffer's address and the reset's switch again: scalars held over the loop cost it spill code)
  typedef float __attribute__((address_space(1)))* gpush;
  PushSet PS;
  float push_old = 0.0f, push_w = 0.0f;   // push_w: the lane's word of the row (lanes 0..7), stored at the step's end
  if constexpr (PUSH) {
    PS = load_push(P);
    if (PS.out) push_old = ((gpush)PS.out)[(size_t)robot * ORR_PUSH_ROW + 7];
  }
  // CLIPS: the motion time of the next clip change (behind the ring, never staged): read at the start, first used after the sub-steps
  float clip_change = 0.0f;
  if constexpr (CLIPS) clip_change = rec[O(CLIP_CHANGE_TIME)];
  {
    // Non-finite guard, entry half: a NaN in the INCOMING rigid state (POS..QD) does not survive the step - the velocity clamp (+-100,
    // v_med3) and the branch-free inverse trigonometric functions turn NaNs into finite numbers - so it is recorded here, in a spare
    // word of the LDS image behind the state head (never stored), and ORed into the exit half of the guard (ORR_DONE_NAN below).
    static_assert(kHead > ORR_OFF_RING, "spare LDS word behind the state head (the head = everything in front of the ring)");
    bool bad_in = false;
    for (int i = lane; i < 37; i += kLanes) bad_in = bad_in || !(fabsf(S.s[O(POS) + i]) < 1e30f);
    const bool any_bad = ((__ballot(bad_in) >> (sub * kLanes)) & ((1ull << (kLanes - 1)) * 2ull - 1ull)) != 0ull;
    if (lane == 0) S.s[kHead - 1] = any_bad ? 1.0f : 0.0f;
  }
  // impulse-response table: stale rows are multiplied by zero impulses, so they only have to be finite
  for (int i = lane; i < kMaxRows * kWStride; i += kLanes) (&S.ph.sub.W[0][0])[i] = 0.0f;
  WSYNC();
  LegConst K;
  load_leg_const(P, S, lane, K);
  {
    float rel[4], Rb[9];
    base_rotation(S, lane, rel, Rb);  // Shared::Rb for the first sub-step; the ring push keeps it current afterwards
  }
  // friction anchors (ANCHOR variant only): the cached contact point of the lane's leg, from the record's words behind the ring
  AnchorState AS = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0};
  bool anchor_robot = false;
  const int aleg = lane < 4 ? lane : (lane < 8 ? lane - 4 : (lane - 8) >> 1);   // leg of the lane's bank-A row (knee, normal, friction)
  if constexpr (ANCHOR) {
    static_assert(kLanes == 16, "ANCHOR: aleg indexes the record's four cached points by the 16-lane row layout");
    anchor_robot = model_cold(P, geti(S, O(ROBOT_TYPE)))->friction_anchor != 0;
    const float* an = rec + O(ANCHOR) + 6 * aleg;
    AS.la[0] = an[0]; AS.la[1] = an[1]; AS.la[2] = an[2]; AS.wb[0] = an[3]; AS.wb[1] = an[4]; AS.wb[2] = an[5];
    AS.valid = anchor_robot ? __float_as_int(rec[O(ANCHOR_VALID) + aleg]) : 0;
  }
  auto store_anchor = [&]() __attribute__((always_inline)) {      // the normal-row lanes (4..7) own the record's words
    if constexpr (ANCHOR) {
      if (valid && lane >= 4 && lane < 8) {
        float* an = rec + O(ANCHOR) + 6 * aleg;
        an[0] = AS.la[0]; an[1] = AS.la[1]; an[2] = AS.la[2]; an[3] = AS.wb[0]; an[4] = AS.wb[1]; an[5] = AS.wb[2];
        rec[O(ANCHOR_VALID) + aleg] = __int_as_float(AS.valid);
      }
    }
  };
  // CONTACTS: lane l < 12 owns LAMBDA word l = (leg l / 3, direction l % 3: normal, friction x, friction y); lanes 12..15 repeat word 0.
  // The sum over the launch's sub-steps and the largest single value (read from the normal lanes only), both from 0
  typedef float __attribute__((address_space(1)))* gcontact;
  const int cw = lane < 12 ? lane : 0;
  float c_sum = 0.0f, c_max = 0.0f;
  auto accumulate_contacts = [&]() __attribute__((always_inline)) {      // behind physics_substep's closing WSYNC
    if constexpr (CONTACTS) {
      const float lw = S.s[O(LAMBDA) + cw];
      c_sum += lw;
      c_max = fmaxf(c_max, lw);
    }
  };
  auto store_contacts = [&]() __attribute__((always_inline)) {           // row [leg][sum n, sum t1, sum t2, max n]: the normal lanes store two words
    if constexpr (CONTACTS) {
      if (valid && lane < 12 && contacts_bound) {
        const int cleg = lane / 3, cd = lane - 3 * cleg;
        gcontact const row = (gcontact)P.tab->contact_out + (size_t)robot * 16 + 4 * cleg;
        row[cd] = c_sum;
        if (cd == 0) row[3] = c_max;
      }
    }
  };
  PT(0);

  if ((MODE & 3) == 1) {
    if (lane < 12) {
      const ColdPtr mc = model_cold(P, geti(S, O(ROBOT_TYPE)));
      const int j = mc->joint_of_motor[lane];
      S.tau[j] = mc->tau_sign_motor[lane] * actions[(size_t)robot * 12 + lane];
    }
    WSYNC();
    int fall = 0;
    OwnCoord X;
    load_own_coord(S, lane, X);
    int limit_idle = 0;
    for (int s = 0; s < nsub; s++) {
      fall = physics_substep<ANCHOR>(P, S, K, lane, sub, true, X, limit_idle, ANCHOR ? &AS : nullptr, anchor_robot);
      accumulate_contacts();
      float rel[4], Rb[9];
      base_rotation(S, lane, rel, Rb);
      WSYNC();
    }
    if (valid && lane == 0 && done_out) done_out[robot] = (uint8_t)fall;
    store_robot(rec, S, lane, valid);
    store_anchor();
    store_contacts();
    return;
  }

  // per-motor constants of the PD loop (lane = motor; lanes 12..15 repeat motor 0), from the cold model table into registers: issued
  // here, first used after the control observation's ring reads
  const int ml = lane < 12 ? lane : 0;
  const ColdPtr mc = model_cold(P, geti(S, O(ROBOT_TYPE)));
  const int mj = mc->joint_of_motor[ml];
  const float m_off = mc->motor_offset[ml], m_dir = mc->motor_dir[ml], m_kp = mc->kp[ml], m_kd = mc->kd[ml];
  const float m_tsign = mc->tau_sign_motor[ml], m_init = mc->init_motor_angles[ml];
  // ACT: the torque limit of the lane's motor, and the launch's accumulators of its motor-convention torque (a_tau: the sub-step's)
  typedef float __attribute__((address_space(1)))* gact;
  float a_lim = INFINITY, a_tau = 0.0f, a_s1 = 0.0f, a_pk = 0.0f, a_s2 = 0.0f, a_w = 0.0f;
  if constexpr (ACT) a_lim = ((const float __attribute__((address_space(1)))*)&P.tab->torque_limit[geti(S, O(ROBOT_TYPE))][0])[ml];
  // SENS: the handle's deviations (scalar), the robot's stream (robot index, episode) and the step's first block for the lane's motor
  SensorNoise SN;
  uint32_t sn_robot = 0u, sn_ep = 0u, sn_i = 0u;
  if constexpr (SENS) {
    SN = load_sensor_noise(P);
    sn_robot = (uint32_t)geti(S, O(ROBOT_INDEX)); sn_ep = (uint32_t)geti(S, O(EPISODE_IDX)); sn_i = 1u + (uint32_t)geti(S, O(EP_STEP));
  }
  // ---- set_act (minitaur.py:280-285): offset, last action, Butterworth filter ----
  ctrl_obs(P, rec, S, lane);
  // Non-finite guard, action half: the +-0.2 rad clip of the motor command (fmin / fmax) would silently DROP a NaN action while the
  // last-action sensor and the filter history keep it.  A non-finite action is recorded like a non-finite incoming state (ORR_DONE_NAN
  // at the end of the step) and replaced by 0, so that nothing non-finite enters the record.
  float act_in = actions[(size_t)robot * 12 + ml];
  {
    const bool bad_act = !(fabsf(act_in) < 1e30f);
    if (bad_act) act_in = 0.0f;
    const bool any_bad = ((__ballot(bad_act) >> (sub * kLanes)) & ((1ull << (kLanes - 1)) * 2ull - 1ull)) != 0ull;
    if (lane == 0 && any_bad) S.s[kHead - 1] = 1.0f;
  }
  if (lane < 12) {
    const float act = act_in + m_init;
    S.s[O(LAST_ACTION) + lane] = act;
    float x1 = S.s[O(XHIST) + lane], x2 = S.s[O(XHIST) + 12 + lane], y1 = S.s[O(YHIST) + lane], y2 = S.s[O(YHIST) + 12 + lane];
    if (geti(S, O(STATE_ACTION_COUNTER)) == 0) {  // _filter (minitaur.py:1169-1178): init_history(current delayed angles)
      float d = map_pi(S.co[lane]);
      if constexpr (SENS) {   // get_motor_angles' reading, with a draw of its own (slot 18)
        if (SN.a > 0.0f) {
          float u4[4], z0, z1;
          philox_block(c.seed, sn_robot, sn_ep, sensor_block(sn_i, kSensorSlotFilter, (uint32_t)lane), u4);
          normal_pair(u4[0], u4[1], &z0, &z1);
          d = map_pi(fmaf(SN.a, z0, S.co[lane]));
        }
      }
      x1 = x2 = y1 = y2 = d;
    }
    const float y = act * P.fb[0] + (x1 * P.fb[1] + x2 * P.fb[2]) - (y1 * P.fa[1] + y2 * P.fa[2]);  // action_filter.py:111-120
    S.s[O(XHIST) + 12 + lane] = x1; S.s[O(XHIST) + lane] = act;
    S.s[O(YHIST) + 12 + lane] = y1; S.s[O(YHIST) + lane] = y;
    S.s[O(ACTION) + lane] = y;
  }
  // PUSH (orr_set_push; draw rule in include/openroborl_hip.h): the kick of this step, on the LDS image before anything reads the rigid
  // state for the first sub-step.  Every lane of the robot evaluates the same blocks (no divergence; block B behind a wave-uniform
  // test, like the sensor variant's of its deviation); lane k < 6 owns word k of LINVEL / ANGVEL.  A robot that is not kicked keeps its
  // words by a select, not by + 0: the sign of a -0.0 passes
  if constexpr (PUSH) {
    static_assert(ORR_OFF_ANGVEL == ORR_OFF_LINVEL + 3, "LINVEL and ANGVEL are six consecutive words");
    const uint32_t ps = sn_i - 1u;   // EP_STEP before the step
    float ua[4], ub[4] = {0.5f, 0.5f, 0.5f, 0.5f};
    philox_block(c.seed, sn_robot, sn_ep, kPushBlock + 2u * ps, ua);
    const bool kicked = (int)ps >= PS.grace && ua[0] < PS.prob;
    float sn, cs;
    unit_sincos(ua[1], &sn, &cs);
    const float pm = fmaf(ua[2], PS.span, PS.lin_lo);
    if (PS.ang > 0.0f) philox_block(c.seed, sn_robot, sn_ep, kPushBlock + 2u * ps + 1u, ub);
    const float two_ang = PS.ang > 0.0f ? 2.0f * PS.ang : 0.0f;   // ang = 0: fmaf(0.5, 0, -0) = 0
    const float mine = lane == 0 ? __fmul_rn(pm, cs) : (lane == 1 ? __fmul_rn(pm, sn) : (lane == 2 ? fmaf(ua[3], 2.0f * PS.lin_z, -PS.lin_z)
                       : fmaf(lane == 3 ? ub[0] : (lane == 4 ? ub[1] : ub[2]), two_ang, -PS.ang)));
    const float dk = kicked && lane < 6 ? mine : 0.0f;
    if (lane < 6) {
      const float v = S.s[O(LINVEL) + lane];
      S.s[O(LINVEL) + lane] = kicked ? __fadd_rn(v, dk) : v;
    }
    const float one = kicked ? 1.0f : 0.0f;
    push_w = lane < 6 ? dk : (lane == 6 ? one : (ps == 0u ? 0.0f : push_old) + one);
  }
  WSYNC();
  PT(1);
  int fall = 0;
  const float inv_repeat = 1.0f / (float)c.action_repeat;
  const RingLatency rlat = ring_latency(P, S);
  // the step's filtered target and the motor gain, in registers over the sub-steps (lane = motor)
  const float m_gain = m_tsign * S.s[O(STRENGTH) + ml];
  const float m_target = S.s[O(ACTION) + ml], m_prev = S.s[O(FILTER_ACTION) + ml];
  const bool m_has_prev = geti(S, O(FILTER_VALID)) != 0;
  int action_counter = geti(S, O(STATE_ACTION_COUNTER));
  RingCursor ring = {geti(S, O(RING_HEAD)), geti(S, O(RING_LEN))};
  OwnCoord X;
  load_own_coord(S, lane, X);
  int limit_idle = 0;      // see physics_substep
  // Two waves per SIMD: VALU issue is arbitrated by priority, then AGE - the older wave of a SIMD runs nearly unimpeded, the younger on
  // the leftover slots, and when the older one has finished the younger runs on alone at a lone wave's pace (half the SIMD idle).  The
  // two waves of a SIMD come from consecutive dispatch rounds (workgroup b: round b / #SIMDs), so raising the priority of the even rounds
  // in even sub-steps and of the odd rounds in odd sub-steps lets them take turns at being the favoured one and finish together.
  // 8192 robots: 0.349 -> 0.331 ms (-5.3 %, round 3; turns of 2 or 4 sub-steps or a second flip in the middle of a sub-step were no
  // better then: 0.332 / 0.332 / 0.335).  Round 4, final code: turns of FOUR sub-steps 0.3015 -> 0.2991 ms (2: 0.2995, 8 / 16: 0.3032 /
  // 0.3027; without the alternation 0.317; profiles/r04_ab25..28_8192.log).
  const int prio_phase = WPE == 2 ? (int)(((unsigned)wave_id / (unsigned)(P.simds > 0 ? P.simds : 1)) & 1u) : 0;
  // Taking turns pairs the dispatch rounds (0, 1), (2, 3) ...: with an ODD number of rounds the last one has no partner of its own, and the
  // plain age order - the oldest wave of a SIMD runs at nearly a lone wave's pace, the next one moves up when it ends - is the better
  // pipeline (12288 robots = 3 rounds: 0.4925 -> 0.4693 ms without the turns; 16384 / 32768 robots = 4 / 8 rounds: 0.5767 / 1.103 ms with
  // them against 0.5847 / 1.109 without; profiles/r04_ab34_large.log)
  const bool prio_turns = WPE == 2 && ((((unsigned)gridDim.x + (unsigned)(P.simds > 0 ? P.simds : 1) - 1u) /
                                        (unsigned)(P.simds > 0 ? P.simds : 1)) & 1u) == 0u;
  // What the PD law of a sub-step reads - the delayed angle of the lane's motor (control observation), the joint's true angle and rate -
  // is produced at the END of the previous sub-step: the control-observation word by this very lane, angle and rate by the integration
  // (read from LDS there anyway, for the ring entry).  Carried over in registers, the top of the loop has no LDS round
  // trip of its own: a lone wave has nothing to overlap one with there.  Same values, bit for bit.  4096 robots 0.2235 -> 0.2205 ms.
  // The two-wave build lost 1 % with it when it was introduced (8192 robots 0.3130 -> 0.3160 ms: three more registers across the sub-step)
  // and takes it since the end of round 4: a wave pair runs 1.33 x the LONE time of its build whatever the scheduling (DESIGN.md section
  // 10), and on the final code the carry is worth 0.3014 -> 0.2991 ms (profiles/r04_ab39_8192.log).  Measured and NOT kept in the one-wave build:
  // carrying the base rotation the same way (nine words that leg_dynamics reads back from LDS: 0.2206, neutral), and issuing the loads
  // of the leg dynamics' first reads (base rotation / velocity, own joint angle, the leg's joint rates: 19 registers) in front of the
  // PD law (0.2208 -> 0.2223: worse).
  float co_own = S.co[ml], qm_c = (S.s[O(Q) + mj] - m_off) * m_dir, qdm_c = S.s[O(QD) + mj] * m_dir;
  const uint32_t sn_blk = sensor_block(sn_i, 0u, (uint32_t)ml);
  float sn_u2 = 0.0f, sn_u3 = 0.0f;    // SENS: words 2, 3 of the even sub-step's block, for the odd one
  for (int sstep = 0; sstep < c.action_repeat; sstep++) {
    // priority turns of the two-wave variant (measured: profiles/r04_ab25..30_8192.log): a wave is favoured for kPrioTurn sub-steps at a time; the turns
    // start kPrioOffset sub-steps early, i.e. the younger wave of a SIMD leads with a turn of three and has the last two sub-steps (8192 robots
    // 0.3012 -> 0.2998 ms; offsets 2 / 3 / 4 (= the older wave leads): 0.3030 / 0.3042 / 0.3046; equal priority for the last 4 / 8 sub-steps:
    // 0.3026 / 0.3014, not kept).  kPrioEqualFrom: equal priority from that sub-step on; 1000 = never (action_repeat is 33), the comparison
    // stays so that the unit's code is the measured one
    constexpr int kPrioTurn = 4, kPrioHi = 1, kPrioOffset = 1, kPrioEqualFrom = 1000;
    if (WPE == 2 && prio_turns) { if (sstep < kPrioEqualFrom && ((((sstep + kPrioOffset) / kPrioTurn) ^ prio_phase) & 1)) __builtin_amdgcn_s_setprio(kPrioHi); else __builtin_amdgcn_s_setprio(0); }
    {  // every lane (no divergent `if`: it would cost more than it skips); lanes 12..15 repeat motor 0 and store into dump slots
      const float lerp = (float)(sstep + 1) * inv_repeat;  // process_action (minitaur.py:438-460)
      float cur = map_pi(co_own), cur_lerp = cur;
      if constexpr (SENS) {
        if (SN.a > 0.0f) {   // wave-uniform, like the test of the sub-step's parity
          float ua, ub, z0, z1;
          if ((sstep & 1) == 0) {
            float u4[4];
            philox_block(c.seed, sn_robot, sn_ep, sn_blk + ((uint32_t)(sstep >> 1) << 4), u4);
            ua = u4[0]; ub = u4[1]; sn_u2 = u4[2]; sn_u3 = u4[3];
          } else {
            ua = sn_u2; ub = sn_u3;
          }
          normal_pair(ua, ub, &z0, &z1);
          cur = map_pi(fmaf(SN.a, z0, co_own));        // _clip_motor_commands' reading
          cur_lerp = map_pi(fmaf(SN.a, z1, co_own));   // process_action's, redrawn every sub-step
        }
      }
      const float prev = m_has_prev ? m_prev : cur_lerp;
      float cmd = prev + lerp * (m_target - prev);
      cmd = fminf(fmaxf(cmd, cur - c.max_angle_change), cur + c.max_angle_change);  // _clip_motor_commands (:706-723)
      // MotorModel.convert_to_torque, POSITION mode (minitaur_motor.py:163-171); pd latency 0 (:359-363): the carried angle and rate
      float tq = m_gain * (-1.0f * (m_kp * (qm_c - cmd)) - m_kd * qdm_c);
      if constexpr (ACT) {   // strength first, then the clip (minitaur_motor.py:165-171; |m_tsign| = 1); selects: without a limit the bits pass
        tq = tq > a_lim ? a_lim : (tq < -a_lim ? -a_lim : tq);
        a_tau = tq * m_tsign;
        a_s1 += a_tau;
        a_pk = fmaxf(a_pk, fabsf(a_tau));
        a_s2 = fmaf(a_tau, a_tau, a_s2);
      }
      S.tau[lane < 12 ? mj : lane] = tq;
    }
    WSYNC();
    action_counter++;  // robot_step bookkeeping (minitaur.py:287-293); written back after the loop
    PT(2);
    {  // receive_obs, then the control observation of the next sub-step / of get_obs
      RingFetch F;
      ring_prefetch(rlat, rec, ring, lane, F);
      if constexpr ((MODE & 3) == 2) {
        const size_t slot = (size_t)robot * c.action_repeat + sstep;
        if (lane < 12 && valid) RP.tau_out[slot * 12 + lane] = S.tau[mj] * m_tsign;  // motor torque, motor order
        WSYNC();
        for (int i = lane; i < 37; i += kLanes) S.s[O(POS) + i] = RP.traj[slot * 37 + i];        // POS QUAT LINVEL ANGVEL Q QD
        WSYNC();
        fall = RP.fall[robot];
      } else
      fall = physics_substep<ANCHOR>(P, S, K, lane, sub, sstep == c.action_repeat - 1, X, limit_idle, ANCHOR ? &AS : nullptr, anchor_robot);
      accumulate_contacts();
      qm_c = (S.s[O(Q) + mj] - m_off) * m_dir;
      qdm_c = S.s[O(QD) + mj] * m_dir;
      if constexpr (ACT) a_w = fmaf(a_tau, qdm_c, a_w);   // sim_dt qd = the sub-step's change of the angle: the work, scaled after the loop
      ring_push_and_ctrl_obs(rec, S, lane, valid, F, ring, qm_c, &co_own);
    }
    PT(10);
  }
  // past its sub-step loop (reward, observation, reset, store: few vector instructions between long memory waits) a wave issues ahead of its
  // partner: it costs the partner next to nothing and shortens the tail (8192 robots: -0.1 %; with -Os for this unit -0.4 %, profiles/r04_ab29_8192.log)
  if (WPE == 2) __builtin_amdgcn_s_setprio(3);
  // the cold-table constants of an auto-reset (ResetConst), issued here, with the step end's other loads (every store and atomic of
  // the step comes behind the reset).  Loaded again rather than taken from the registers that hold some of them over the sub-steps
  // (m_init is dead by now): keeping those live up to the reset moved the sub-step loop's register allocation (+10 instructions) for
  // a launch no faster
  const ResetConst RC = load_reset_const(P, S, lane);
  float* push_out = nullptr;     // PUSH: the outputs buffer and the reset's switch, read again (see PS)
  bool push_table = false;
  if constexpr (PUSH) load_push_end(P, &push_out, &push_table);
  if (lane == 0) {  // end of robot_step (minitaur.py:287-293)
    seti(S, O(RING_HEAD), ring.head); seti(S, O(RING_LEN), ring.len);
    seti(S, O(STATE_ACTION_COUNTER), action_counter);
    seti(S, O(FILTER_VALID), 1);
    seti(S, O(STEP_COUNTER), geti(S, O(STEP_COUNTER)) + 1);
  }
  if (lane < 12) S.s[O(FILTER_ACTION) + lane] = m_target;
  WSYNC();
  // ---- get_obs: sensors on_step (minitaur.py:295-299) ----
  if constexpr (SENS) sensors_push_noisy(S, lane, false, SN, c.seed, sn_ep, sn_i);
  else sensors_push(S, lane, false);
  PT(11);
  // ---- reward -> update -> done (quadruped_gym_env.py:230-233) ----
  // the frames of the new reference poses are fetched while the reward is computed (their round trip to L2 is not waited for)
  const DevClip& clip = S.clip;
  double t = motion_time(P, S);                             // f64: see DevClip
  // CLIPS: the clip change of _update_ref_motion (imitation_task.py:734-761, 1096-1101), decided before anything samples the clip.  The
  // phase of the update is the NEW clip's at the OLD offset's time (t_phase, :749-750); pose, targets and termination use the new time
  double t_phase = t;
  bool switched = false;
  if constexpr (CLIPS) {
    if (t >= (double)clip_change) {
      typedef const int __attribute__((address_space(1)))* gip;
      typedef const float __attribute__((address_space(1)))* gfp;
      const int type = geti(S, O(ROBOT_TYPE));
      const int set_n = ((gip)&P.tab->clip_set_n[0])[type];
      const float sw_min = ((gfp)&P.tab->clip_switch[type][0])[0], sw_max = ((gfp)&P.tab->clip_switch[type][0])[1];
      // num_motions > 1 (:1099), and the type still has an interval: switching turned off (orr_set_clip_switch(+inf, +inf)) stops at once,
      // although the records keep their finite change times until their next reset
      if (set_n > 1 && sw_max < INFINITY) {
        // draws 32 + 4 s .. 34 + 4 s of the episode's stream (Philox block 8 + s, s = the env step counter before this step): the clip
        // (as reset_robot_state<true> draws it), the next change, the new time offset (_sample_time_offset, :1112-1123)
        // The lane that holds the drawn entry writes CLIP_ID (clip_drawn: the thresholds' rule), and every lane reads it back
        const ClipDraw cdraw = clip_draw_issue(P, type, lane);
        float u4[4];
        philox_block(c.seed, (uint32_t)geti(S, O(ROBOT_INDEX)), (uint32_t)geti(S, O(EPISODE_IDX)), 8u + (uint32_t)geti(S, O(EP_STEP)), u4);
        const uint32_t m = (uint32_t)(u4[0] * 16777216.0f);
        clip_change = clip_change_time(t, sw_min, sw_max, u4[1]);
        WSYNC();
        if (clip_drawn(cdraw, m, lane)) seti(S, O(CLIP_ID), cdraw.set_id);
        WSYNC();
        const int id = geti(S, O(CLIP_ID));
        const unsigned int* cg = reinterpret_cast<const unsigned int*>(&P.tab->clip[id]);
        unsigned int* cl = reinterpret_cast<unsigned int*>(&S.clip);
        if (lane < (int)(sizeof(DevClip) / 4)) cl[lane] = cg[lane];
        WSYNC();
        if (lane == 0) {
          S.s[O(TIME_OFFSET)] = u4[2] * (float)clip.dur_d;
          if (valid) rec[O(CLIP_CHANGE_TIME)] = clip_change;   // an auto-reset later in this step overwrites it (same lane, in order)
        }
        WSYNC();
        t = motion_time(P, S);
        switched = true;
      }
    }
  }
  const double step_dt = clip.sim_dt_d * c.action_repeat;
  double tl = t;
  if (lane >= 1 && lane <= 4) tl = t + target_frame_steps(c, lane) * step_dt;   // lanes 1..4: the four target times
  PoseLoads PL;
  sample_poses_issue(P, S, lane, tl, PL);
  // TERMS: lanes 0..4 own the robot's row of running sums (one term each); its load is issued here, with the frame loads, and first used
  // at the step's end.  A padding lane group shadows robot 0: it loads that row and never stores
  typedef float __attribute__((address_space(1)))* gterm;
  float term = 0.0f, term_sum = 0.0f;
  if constexpr (TERMS) {
    if (lane < 5 && terms_bound) term_sum = ((gterm)P.tab->term_sums)[(size_t)robot * 5 + lane];
  }
  // CONTACTS: lanes 0..7 own the robot's row of episode totals ([leg][stance steps, sum of the normal sums]); loaded here likewise
  float c_ep = 0.0f;
  if constexpr (CONTACTS) {
    if (lane < 8 && contacts_bound) c_ep = ((gcontact)P.tab->contact_ep)[(size_t)robot * 8 + lane];
  }
  // ACT: lanes 0..3 own the robot's row of episode totals (work, sum tau^2, largest |tau|, saturated steps); loaded here likewise.  Env step only
  float a_ep = 0.0f;
  if constexpr (ACT && (MODE & 3) == 0) {
    if (lane < 4 && act_bound) a_ep = ((gact)P.tab->act_ep)[(size_t)robot * 4 + lane];
  }
  float rew;
  if constexpr (TERMS) {
    float tk[5];
    rew = calc_reward<true>(P, S, lane, (MODE & 3) == 2 ? RP.eff + (size_t)robot * 48 : nullptr, tk);
    term = lane == 0 ? tk[0] : (lane == 1 ? tk[1] : (lane == 2 ? tk[2] : (lane == 3 ? tk[3] : tk[4])));
  } else {
    rew = calc_reward(P, S, lane, (MODE & 3) == 2 ? RP.eff + (size_t)robot * 48 : nullptr);
  }
  sample_poses_finish(P, S, lane, tl, true, PL);
  {
    // _update_ref_motion (imitation_task.py:734-761) with _sync_ref_origin (:1020-1055)
    const float ph = clip_phase(clip, t_phase);
    if (lane == 0) {
      bool sync_pos = (c.flags & ORR_FLAG_CYCLE_SYNC) && ph < S.s[O(PREV_PHASE)];
      if constexpr (CLIPS) {
        if (switched) {   // a clip change syncs the heading (relative to the init orientation, _calc_heading) first, then the position
          q_about_z(task_heading(S, &S.s[O(QUAT)]) - task_heading(S, &S.ph.end.pose[0][3]), &S.s[O(ORIGIN_ROT)]);
          sync_pos = true;
        }
      }
      if (sync_pos) {
        float pr[3];
        qrot(&S.ph.end.pose[0][0], &S.s[O(ORIGIN_ROT)], pr);
        S.s[O(ORIGIN_POS)] = S.s[O(POS)] - pr[0];
        S.s[O(ORIGIN_POS) + 1] = S.s[O(POS) + 1] - pr[1];
        S.s[O(ORIGIN_POS) + 2] = 0.0f;
      }
      S.s[O(PREV_PHASE)] = ph;
      float v[3];
      qrot(&S.ph.end.vel[0], &S.s[O(ORIGIN_ROT)], v); S.ph.end.vel[0] = v[0]; S.ph.end.vel[1] = v[1]; S.ph.end.vel[2] = v[2];
      qrot(&S.ph.end.vel[3], &S.s[O(ORIGIN_ROT)], v); S.ph.end.vel[3] = v[0]; S.ph.end.vel[4] = v[1]; S.ph.end.vel[5] = v[2];
    }
    WSYNC();
    apply_origin(S, lane, 5);
    for (int i = lane; i < 19; i += kLanes) S.s[O(REF_POSE) + i] = S.ph.end.pose[0][i];
    for (int i = lane; i < 18; i += kLanes) S.s[O(REF_VEL) + i] = S.ph.end.vel[i];
    WSYNC();
  }
  PT(12);
  // _terminal_condition (imitation_task.py:518-572) + time limit (wrapper_env.py:79) + non-finite guard
  int reason = 0;
  uint32_t noise_i = 0u;     // NOISE: 1 + the env-step counter before this step (target_obs<true>)
  {
    const float* rp = &S.s[O(REF_POSE)];
    float pe = 0.0f, qc[4], dq[4];
#pragma unroll
    for (int k = 0; k < 3; k++) { float d = rp[k] - S.s[O(POS) + k]; pe += d * d; }
    qconj(&S.s[O(QUAT)], qc);
    qmul(rp + 3, qc, dq);
    const float ang = q_norm_angle(dq);
    if (geti(S, O(STEP_COUNTER)) > 0 && fall) reason |= ORR_DONE_CONTACT_FALL;
    if (pe > c.dist_fail_threshold * c.dist_fail_threshold) reason |= ORR_DONE_ROOT_POS;
    if (fabsf(ang) > c.rot_fail_threshold) reason |= ORR_DONE_ROOT_ROT;
    if (!(clip.flags & ORR_CLIP_WRAP) && t >= clip.dur_d) reason |= ORR_DONE_MOTION_OVER;  // is_motion_over (:224-233)
    bool bad = false;
    for (int i = lane; i < 37; i += kLanes) bad = bad || !(fabsf(S.s[O(POS) + i]) < 1e30f);
    if (((__ballot(bad) >> (sub * kLanes)) & ((1ull << (kLanes - 1)) * 2ull - 1ull)) != 0ull || S.s[kHead - 1] != 0.0f) reason |= ORR_DONE_NAN;
    if (!(fabsf(rew) < 1e30f)) reason |= ORR_DONE_NAN;
    if (reason & ORR_DONE_NAN) rew = 0.0f;      // whatever was computed from a non-finite state is not a reward
    const int ep_step = geti(S, O(EP_STEP)) + 1;  // quadruped_gym_env.py:237
    if constexpr (TERMS) {   // the first step of an episode restarts the sums (no reset kernel touches them); a non-finite step counts as five zeros
      if (reason & ORR_DONE_NAN) term = 0.0f;
      term_sum = (ep_step == 1 ? 0.0f : term_sum) + term;
    }
    if constexpr (CONTACTS) {   // likewise; a non-finite step counts as sixteen zeros.  Lane 2 leg + k gets the leg's normal sum from lane 3 leg
      if (reason & ORR_DONE_NAN) c_sum = c_max = 0.0f;
      const float nsum = __shfl(c_sum, sub * kLanes + 3 * ((lane & 7) >> 1));
      const float add = nsum > 0.0f ? ((lane & 1) ? nsum : 1.0f) : 0.0f;
      c_ep = (ep_step == 1 ? 0.0f : c_ep) + add;
    }
    if constexpr (ACT) {   // likewise; a non-finite step counts as zeros.  The twelve motors' totals by row reductions, lanes 12..15 (motor 0 again) as 0
      a_w *= c.sim_dt;
      if (reason & ORR_DONE_NAN) a_s1 = a_pk = a_s2 = a_w = 0.0f;
      if constexpr ((MODE & 3) == 0) {
        const bool motor = lane < 12;
        const float w_all = row_sum16(motor ? a_w : 0.0f), s2_all = row_sum16(motor ? a_s2 : 0.0f), pk_all = row_max16(motor ? a_pk : 0.0f);
        const float sat_all = row_max16(motor && !(reason & ORR_DONE_NAN) && a_pk == a_lim ? 1.0f : 0.0f);
        const float old = ep_step == 1 ? 0.0f : a_ep;
        a_ep = lane == 2 ? fmaxf(old, pk_all) : old + (lane == 0 ? w_all : (lane == 1 ? s2_all : sat_all));
      }
    }
    if constexpr (NOISE) noise_i = (uint32_t)ep_step;
    if (ep_step >= geti(S, O(MAX_EP_STEPS))) reason |= ORR_DONE_TIME_LIMIT;
    WSYNC();
    if (lane == 0) {
      seti(S, O(EP_STEP), ep_step);
      seti(S, O(DONE_REASON), reason);
      S.s[O(EP_RETURN)] += rew;
    }
  }
  PT(13);
  // ---- episode end: what the log row needs, then the inline auto-reset.  From here to the stores below NOTHING is stored and no
  // atomic is issued: loads, stores and atomics share one in-order counter (vmcnt), so the reset's wait for its clip frames would sit
  // out the round trip of whatever store or atomic was issued in front of it (the episode-log atomic: several microseconds) ----
  float log_ret = 0.0f, log_len = 0.0f;
  int log_clip = 0;     // CLIPS: the clip the ending episode played, read before the reset draws the next one
  uint32_t obs_episode = (uint32_t)geti(S, O(EPISODE_IDX));
  bool was_reset = false;
  if (reason != 0) {
    if (lane == 0) {
      log_ret = S.s[O(EP_RETURN)]; log_len = (float)geti(S, O(EP_STEP));
      if constexpr (CLIPS) log_clip = geti(S, O(CLIP_ID));
      S.s[O(LAST_EP_RETURN)] = log_ret;
      seti(S, O(LAST_EP_LEN), geti(S, O(EP_STEP)));
    }
    WSYNC();
    if (c.flags & ORR_FLAG_AUTO_RESET) {
      PT(31);
      // PUSH: a handle without a randomiser table or params buffer keeps the reset it had (the literal ranges: the table-driven form of
      // the same ranges rounds hi - lo once more); wave-uniform
      if constexpr (PUSH) {
        if (push_table) obs_episode = reset_robot_state<CLIPS, NOISE, SENS, true>(P, S, lane, total_snapshot, RC, &clip_change, nullptr, SN, &RR);
        else obs_episode = reset_robot_state<CLIPS, NOISE, SENS>(P, S, lane, total_snapshot, RC, &clip_change, nullptr, SN);
      } else
      if constexpr (RAND) obs_episode = reset_robot_state<CLIPS, NOISE, SENS, true>(P, S, lane, total_snapshot, RC, &clip_change, nullptr, SN, &RR);
      else obs_episode = reset_robot_state<CLIPS, NOISE, SENS>(P, S, lane, total_snapshot, RC, &clip_change, nullptr, SN);
      noise_i = 0u;
      was_reset = true;
      if constexpr (ANCHOR) AS = AnchorState{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0};   // a new episode: no cached contact points
    }
  }
  WSYNC();
  PT(14);
  // ---- observation (wrapper_env.py:109-125), ONCE per robot: of the step that ended, or of the episode that just began ----
  build_obs<NOISE, SENS>(P, rec, S, lane, obs, obs_episode, noise_i, SN);
  PT(13);
  // ---- every store of the step, behind every load ----
  if (valid && lane == 0) {
    reward_out[robot] = rew;
    done_out[robot] = reason != 0;
  }
  if constexpr (TERMS) {
    if (valid && lane < 5 && terms_bound) {
      ((gterm)P.tab->terms)[(size_t)robot * 5 + lane] = term;
      ((gterm)P.tab->term_sums)[(size_t)robot * 5 + lane] = term_sum;
    }
  }
  if constexpr (CONTACTS) {
    store_contacts();
    if (valid && lane < 8 && contacts_bound) ((gcontact)P.tab->contact_ep)[(size_t)robot * 8 + lane] = c_ep;
  }
  if constexpr (ACT) {   // row [motor] = {sum tau, max |tau|, sum tau^2, work}: one 16-byte store per motor lane
    if (valid && lane < 12 && act_bound) {
      typedef f4 __attribute__((address_space(1)))* gact4;
      ((gact4)reinterpret_cast<f4*>(P.tab->act_out))[(size_t)robot * 12 + lane] = f4{a_s1, a_pk, a_s2, a_w};
    }
    if constexpr ((MODE & 3) == 0) {
      if (valid && lane < 4 && act_bound) ((gact)P.tab->act_ep)[(size_t)robot * 4 + lane] = a_ep;
    }
  }
  if constexpr (PUSH) {   // row = {dv, dw, kicked, kicks of the episode}: what was applied at the start of this step, one word per lane 0..7
    if (valid && lane < ORR_PUSH_ROW && push_out) ((gpush)push_out)[(size_t)robot * ORR_PUSH_ROW + lane] = push_w;
  }
  if (was_reset) store_reset_extras<CLIPS>(rec, S, lane, valid, clip_change);   // ring entries #1 / #2 of the new episode (still in LDS)
  if constexpr (RAND) { if (was_reset) store_rand_row(P, RR, lane, valid); }    // and its row of the params buffer
  store_robot(rec, S, lane, valid);
  store_anchor();
  if (valid) {   // the observation, in 16-byte pieces like the record (40 per robot)
    typedef f4 __attribute__((address_space(1))) * g4ptr;
    static_assert(ORR_OBS_DIM % 4 == 0, "16-byte pieces");
    const g4ptr od = (g4ptr)reinterpret_cast<f4*>(obs_out + (size_t)robot * ORR_OBS_DIM);
    const f4* os = reinterpret_cast<const f4*>(obs);
#pragma unroll
    for (int k = 0; k < (ORR_OBS_DIM / 4 + kLanes - 1) / kLanes; k++) { const int q = lane + k * kLanes; if (q < ORR_OBS_DIM / 4) od[q] = os[q]; }
  }
  PT(15);
  PT_FLUSH();
  // ---- the two returning atomics of the step end, back to back, and ONE wait for both ----
  // Episode log (imitation_runners.py:185-197): lane 0 of a robot whose episode ended takes its slot from a cursor shared by the
  // whole device - whether or not a log is bound: the cursor counts the finished episodes.
  // Launch tally: one counter update per WAVE (the compiler's own atomic combining is switched off, see _lib.HIPCC_FLAGS: it makes the
  // issuing lane wait for the returned value on the spot).  The tally is ONE 64-bit word (ORR_CNT_TICKET: finished episodes in the
  // high half, robots counted in the low half), so one returning atomic both adds the wave's finished episodes and takes its ticket:
  // there is no second word to order it against, and no fence (it cost 7 % of the launch: a write-back of the wave's ~18 KB of fresh
  // stores, an L2 invalidate and two waits).  The wave that completes the count folds the done count into the
  // curriculum counter (wrapper_env.py:82-83) and clears the word with non-returning atomics.  The fold may land while other waves
  // still run: every wave read its snapshot of the curriculum counter when it started, and the last ticket can only be taken once
  // every wave of the launch has started (and taken its own).  The episode log and the records are read after the kernel boundary only.
  // Both are issued HERE, not where the end of the episode becomes known: a returned value held across the reset moved the sub-step
  // loop's register allocation, and an atomic in flight across the reset is waited for by the reset's first load.
  // The values are only defined where the atomics were issued and only read there.  Frozen nondeterministic values instead of
  // uninitialised variables: reading them is defined behaviour in every lane, and unlike a constant they give the compiler nothing to
  // merge with an atomic's result.  The empty asm reads both in every lane: the wait for the two sits in front of it, once.
  const unsigned long long fin_mask = __ballot(valid && lane == 0 && reason != 0), val_mask = __ballot(valid && lane == 0);
  const unsigned long long add = ((unsigned long long)__popcll(fin_mask) << 32) | (unsigned long long)__popcll(val_mask);
  unsigned long long log_slot = __builtin_nondeterministic_value(log_slot), ticket = __builtin_nondeterministic_value(ticket);
  if (lane == 0 && valid && reason != 0) log_slot = atomicAdd((unsigned long long*)&P.counters[ORR_CNT_EPISODES], 1ull);
  // (the two-wave build keeps `wtid` in scratch by now: reloading it between the two atomics would put a wait for the first in front of
  // the second, so that build computes the lane's number afresh)
  const int tally_lane = WPE == 2 ? (int)__lane_id() : wtid;
  if (tally_lane == 0) ticket = atomicAdd((unsigned long long*)&P.counters[ORR_CNT_TICKET], add);
  asm volatile("" : "+v"(log_slot), "+v"(ticket));
  if (reason != 0) {   // the log rows of the ended episode (the cap test and the drop counter: per slot)
    const bool logs = lane == 0 && valid;
    const unsigned long long slot = log_slot;
    if (logs && P.ep_log) {
      if (slot < (unsigned long long)P.ep_log_cap) {
        P.ep_log[2 * slot] = log_ret;
        P.ep_log[2 * slot + 1] = log_len;
        if constexpr (CLIPS) {
          int* const clip_log = P.tab->clip_log;
          if (clip_log) clip_log[slot] = log_clip;
        }
      } else {
        atomicAdd((unsigned long long*)&P.counters[ORR_CNT_EPLOG_DROPPED], 1ull);
      }
    }
    if constexpr (TERMS) {
      // the ending episode's five sums into the log row: the slot lives in lane 0 only, lanes 0..4 get it by a lane broadcast (every lane
      // of the robot is active here: `reason` is uniform over them)
      const int src = sub * kLanes;
      const unsigned long long tslot = ((unsigned long long)(unsigned)__shfl((int)(slot >> 32), src) << 32) | (unsigned)__shfl((int)slot, src);
      gterm const term_log = (gterm)P.tab->term_log;
      if (valid && lane < 5 && P.ep_log && term_log && tslot < (unsigned long long)P.ep_log_cap) term_log[tslot * 5 + lane] = term_sum;
    }
    if constexpr (CONTACTS) {   // the ending episode's contact totals into the log row, lanes 0..7: the slot by a lane broadcast as above
      const int src = sub * kLanes;
      const unsigned long long cslot = ((unsigned long long)(unsigned)__shfl((int)(slot >> 32), src) << 32) | (unsigned)__shfl((int)slot, src);
      gcontact const contact_log = (gcontact)P.tab->contact_log;
      if (valid && lane < 8 && P.ep_log && contact_log && cslot < (unsigned long long)P.ep_log_cap) contact_log[cslot * 8 + lane] = c_ep;
    }
    if constexpr (ACT && (MODE & 3) == 0) {   // the ending episode's actuator totals into the log row, lanes 0..3: likewise
      const int src = sub * kLanes;
      const unsigned long long aslot = ((unsigned long long)(unsigned)__shfl((int)(slot >> 32), src) << 32) | (unsigned)__shfl((int)slot, src);
      gact const act_log = (gact)P.tab->act_log;
      if (valid && lane < 4 && P.ep_log && act_log && aslot < (unsigned long long)P.ep_log_cap) act_log[aslot * 4 + lane] = a_ep;
    }
  }
  if (tally_lane == 0) {
    const unsigned long long now = ticket + add;
    if ((unsigned int)now == (unsigned int)P.cfg.num_robots) {   // the low half never carries: it counts up to num_robots
      atomicAdd((unsigned long long*)&P.counters[ORR_CNT_TOTAL_STEP_COUNT], now >> 32);
      atomicAdd((unsigned long long*)&P.counters[ORR_CNT_TOTAL_TIMESTEPS], (unsigned long long)P.cfg.num_robots);
      atomicExch((unsigned long long*)&P.counters[ORR_CNT_TICKET], 0ull);   // every other wave's update came before this wave's
    }
  }
  WT_STORE((long long)((fin_mask & 1ull) | ((fin_mask >> 15) & 2ull) | ((fin_mask >> 30) & 4ull) | ((fin_mask >> 45) & 8ull)));   // one bit per robot of the wave
}


#ifdef ORR_STAGE_DUMP
// Development aid (tests/test_gpu_substep_stages.py, tools/dev_build.py STAGE_DUMP): -DORR_STAGE_DUMP adds a kernel that runs the FIRST
// HALF of one physics sub-step - leg_dynamics, row_setup_bank_a / row_setup_limit, row_response for both banks, the functions of
// orr_physics.h themselves, called in physics_substep's order with its arguments - on the records as they are and writes what the stages
// hand to each other to a caller's buffer, kStageWords float32 words per robot (integers as values).  Up to the first sub-step it is
// the debug physics (MODE & 3 == 1) of orr_step_kernel; it never stores the record.  The joint-limit bank is always set up and answered
// (no limit_idle skipping, no `anyB` test).  Layout of a robot's words (tests/stage_refs.py mirrors it):
//   kStageUstar   ustar[18]                                          after leg_dynamics
//   kStageLc      lc[12][18]: Rw[9], ow[3], s[3], sv[3]              (dumped before row_response: W shares the space of dyn)
//   kStageLeg     leg[4][24]: T[3][6], Hi[6]
//   kStageBf      per lane 27: the factor L of A0 packed row-wise, (i, j) -> i (i + 1) / 2 + j (its diagonal as 1 / idg: Chol6Pk keeps
//                 the reciprocals only), then idg[6]
//   kStageRow     per lane and bank (A, B) 40: active, leg, nrm_slot, warm, Jb[6], jl[3], rhs (unscaled), cfm, lo_c, hi_c, mu_e after the
//                 setup; wa[6], wq[12], jdi, rhs (scaled), lam, w after the response
//   kStageGeom    per lane 20: ContactGeom[12], the joint-limit margin, AnchorState after the setup (la[3], wb[3], valid; zeros without ANCHOR)
//   kStageW       the LDS copy W[28][18] after the responses
// Whole waves, no data-dependent loop, every store behind a bounds check, a padding lane group stores nothing.
namespace orr {
constexpr int kStageUstar = 0, kStageLc = kStageUstar + 18, kStageLeg = kStageLc + 12 * 18, kStageBf = kStageLeg + 4 * 24;
constexpr int kStageRowWords = 40, kStageRow = kStageBf + kLanes * 27, kStageGeom = kStageRow + kLanes * 2 * kStageRowWords;
constexpr int kStageW = kStageGeom + kLanes * 20, kStageWords = kStageW + kMaxRows * 18;
}
template <bool ANCHOR, int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void orr_stage_dump_kernel(KParams P, const float* torques, float* out, long long out_words) {
  ORR_PROLOGUE();
  (void)obs;
  const bool valid = in_range;
  const orr_config& cfg = P.cfg;
  const long long base = (long long)robot * kStageWords;
  auto put = [&](int k, float v) __attribute__((always_inline)) {
    if (valid && k >= 0 && k < kStageWords && base + k < out_words) out[base + k] = v;
  };
  load_robot(P, rec, S, lane);
  for (int i = lane; i < kMaxRows * kWStride; i += kLanes) (&S.ph.sub.W[0][0])[i] = 0.0f;
  WSYNC();
  LegConst K;
  load_leg_const(P, S, lane, K);
  {
    float rel[4], Rb[9];
    base_rotation(S, lane, rel, Rb);
  }
  AnchorState AS = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0};
  bool anchor_robot = false;
  const int aleg = lane < 4 ? lane : (lane < 8 ? lane - 4 : (lane - 8) >> 1);
  if constexpr (ANCHOR) {
    anchor_robot = model_cold(P, geti(S, O(ROBOT_TYPE)))->friction_anchor != 0;
    const float* an = rec + O(ANCHOR) + 6 * aleg;
    AS.la[0] = an[0]; AS.la[1] = an[1]; AS.la[2] = an[2]; AS.wb[0] = an[3]; AS.wb[1] = an[4]; AS.wb[2] = an[5];
    AS.valid = anchor_robot ? __float_as_int(rec[O(ANCHOR_VALID) + aleg]) : 0;
  }
  if (lane < 12) {
    const ColdPtr mc = model_cold(P, geti(S, O(ROBOT_TYPE)));
    const int j = mc->joint_of_motor[lane];
    S.tau[j] = mc->tau_sign_motor[lane] * torques[(size_t)robot * 12 + lane];
  }
  WSYNC();
  // ---- physics_substep's first half ----
  const float dt = cfg.sim_dt, inv_dt = 1.0f / cfg.sim_dt, erp_dt = cfg.contact_erp / cfg.sim_dt;
  BaseFactor BF;
  leg_dynamics(P, S, K, lane, BF);
  WSYNC();
  for (int i = lane; i < 18; i += kLanes) put(kStageUstar + i, S.ustar[i]);
  for (int i = lane; i < 12 * 18; i += kLanes) {
    const LinkCache& L = S.ph.sub.dyn.lc[i / 18];
    const int k = i % 18;
    put(kStageLc + i, k < 9 ? L.Rw[k] : (k < 12 ? L.ow[k - 9] : (k < 15 ? L.s[k - 12] : L.sv[k - 15])));
  }
  for (int i = lane; i < 4 * 24; i += kLanes) {
    const LegSolve& Q = S.leg[i / 24];
    const int k = i % 24;
    put(kStageLeg + i, k < 18 ? Q.T[k / 6][k % 6] : Q.Hi[k - 18]);
  }
  {
    const Chol6Pk& F = BF.F;
    const float Lp[21] = {1.0f / F.idg[0],
                          F.l10, 1.0f / F.idg[1],
                          F.c0a.x, F.c1a.x, 1.0f / F.idg[2],
                          F.c0a.y, F.c1a.y, F.l32, 1.0f / F.idg[3],
                          F.c0b.x, F.c1b.x, F.c2b.x, F.c3b.x, 1.0f / F.idg[4],
                          F.c0b.y, F.c1b.y, F.c2b.y, F.c3b.y, F.l54, 1.0f / F.idg[5]};
#pragma unroll
    for (int i = 0; i < 21; i++) put(kStageBf + lane * 27 + i, Lp[i]);
#pragma unroll
    for (int i = 0; i < 6; i++) put(kStageBf + lane * 27 + 21 + i, F.idg[i]);
  }
  auto put_setup = [&](int bank, const Row& R) __attribute__((always_inline)) {
    const int o = kStageRow + (lane * 2 + bank) * kStageRowWords;
    put(o, R.active ? 1.0f : 0.0f); put(o + 1, (float)R.leg); put(o + 2, (float)R.nrm_slot); put(o + 3, (float)R.warm);
#pragma unroll
    for (int i = 0; i < 6; i++) put(o + 4 + i, R.Jb[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) put(o + 10 + i, R.jl[i]);
    put(o + 13, R.rhs); put(o + 14, R.cfm); put(o + 15, R.lo_c); put(o + 16, R.hi_c); put(o + 17, R.mu_e);
  };
  auto put_response = [&](int bank, const Row& R) __attribute__((always_inline)) {
    const int o = kStageRow + (lane * 2 + bank) * kStageRowWords + 18;
#pragma unroll
    for (int i = 0; i < 6; i++) put(o + i, R.wa[i]);
#pragma unroll
    for (int i = 0; i < 12; i++) put(o + 6 + i, R.wq[i]);
    put(o + 18, R.jdi); put(o + 19, R.rhs); put(o + 20, R.lam); put(o + 21, R.w);
  };
  Row A, B;
  const bool rowlane = lane < 16;
  ContactGeom G;
  row_setup_bank_a<ANCHOR>(S, cfg, rowlane ? (lane < 4 ? lane : lane + 12) : 0, rowlane, dt, inv_dt, erp_dt, A, G, ANCHOR ? &AS : nullptr, anchor_robot);
  float margin = 1e30f;
  row_setup_limit(S, cfg, (rowlane && lane >= 4) ? lane : 4, rowlane && lane >= 4, inv_dt, erp_dt, B, &margin);
  put_setup(0, A);
  put_setup(1, B);
  {
    const int o = kStageGeom + lane * 20;
    const float g[12] = {G.rr0, G.rr1, G.rr2, G.c00, G.c01, G.c02, G.c10, G.c11, G.c12, G.c20, G.c21, G.c22};
#pragma unroll
    for (int i = 0; i < 12; i++) put(o + i, g[i]);
    put(o + 12, margin);
#pragma unroll
    for (int i = 0; i < 3; i++) { put(o + 13 + i, AS.la[i]); put(o + 16 + i, AS.wb[i]); }
    put(o + 19, (float)AS.valid);
  }
  row_response(S, cfg, A, rowlane ? (lane < 4 ? lane : lane + 12) : 0, BF);
  row_response(S, cfg, B, (rowlane && lane >= 4) ? lane : kMaxRows, BF);   // lanes without a joint-limit row: dump slot
  put_response(0, A);
  put_response(1, B);
  WSYNC();
  for (int i = lane; i < kMaxRows * 18; i += kLanes) put(kStageW + i, S.ph.sub.W[i / 18][i % 18]);
}
#endif

// ================================================================================================
// launchers
// ================================================================================================
// One launcher per kernel template: `waves` = robots / kRPW rounded up, each a workgroup of its own.
// Each instantiation belongs to ONE unit, which instantiates it explicitly (`template orr::StepLaunch orr::launch_step<...>;`, in the
// order its kernels are to have in the code object); the `extern template` declarations below keep every other unit from
// instantiating it, kernel included.
namespace orr {
using StepLaunch = hipError_t(const KParams& P, int waves, hipStream_t stream, const float* actions, float* obs, float* reward, uint8_t* done,
                              int nsub, const ReplayArgs& rp);
using ResetLaunch = hipError_t(const KParams& P, int waves, hipStream_t stream, const uint8_t* mask, float* obs, const float* uniforms);

template <int MODE, int WPE, bool ANCHOR, bool CLIPS, bool NOISE = false>
hipError_t launch_step(const KParams& P, int waves, hipStream_t stream, const float* actions, float* obs, float* reward, uint8_t* done, int nsub,
                       const ReplayArgs& rp) {
  hipLaunchKernelGGL((orr_step_kernel<MODE, WPE, ANCHOR, CLIPS, NOISE>), dim3(waves), dim3(64), 0, stream, P, actions, obs, reward, done, nsub, rp);
  return hipGetLastError();
}
template <bool CLIPS, bool NOISE = false>
hipError_t launch_reset(const KParams& P, int waves, hipStream_t stream, const uint8_t* mask, float* obs, const float* uniforms) {
  hipLaunchKernelGGL((orr_reset_kernel<CLIPS, NOISE>), dim3(waves), dim3(64), 0, stream, P, mask, obs, uniforms);
  return hipGetLastError();
}
template <bool CLIPS>
hipError_t launch_sensor_reset(const KParams& P, int waves, hipStream_t stream, const uint8_t* mask, float* obs, const float* uniforms) {
  hipLaunchKernelGGL((orr_sensor_reset_kernel<CLIPS>), dim3(waves), dim3(64), 0, stream, P, mask, obs, uniforms);
  return hipGetLastError();
}
template <bool CLIPS>
hipError_t launch_randomizer_reset(const KParams& P, int waves, hipStream_t stream, const uint8_t* mask, float* obs, const float* uniforms) {
  hipLaunchKernelGGL((orr_randomizer_reset_kernel<CLIPS>), dim3(waves), dim3(64), 0, stream, P, mask, obs, uniforms);
  return hipGetLastError();
}

extern template StepLaunch launch_step<0, 2, false, false>;                  // orr_kernels_w2.hip
extern template StepLaunch launch_step<0, 1, true, false>;                   // orr_kernels_anchor.hip: env step,
extern template StepLaunch launch_step<1, 1, true, false>;                   //   debug physics
extern template StepLaunch launch_step<0, 1, false, true>;                   // orr_kernels_multiclip.hip: env step,
extern template StepLaunch launch_step<2, 1, false, true>;                   //   its parity replay,
extern template ResetLaunch launch_reset<true>;                              //   reset (and, with the draws given, its parity replay)
extern template StepLaunch launch_step<0, 1, false, true, true>;             // orr_kernels_noise.hip: env step,
extern template StepLaunch launch_step<2, 1, false, true, true>;             //   its parity replay,
extern template ResetLaunch launch_reset<true, true>;                        //   reset (and its parity replay)
extern template StepLaunch launch_step<kModeTerms | 0, 1, false, true, true>;   // orr_kernels_terms.hip: env step with the reward terms,
extern template StepLaunch launch_step<kModeTerms | 2, 1, false, true, true>;   //   its parity replay (resets: the noise unit's)
extern template StepLaunch launch_step<kModeContacts | 0, 1, false, true, true>;                // orr_kernels_contacts.hip: env step with the contact sums,
extern template StepLaunch launch_step<kModeContacts | kModeTerms | 0, 1, false, true, true>;   //   the same with the reward terms,
extern template StepLaunch launch_step<kModeContacts | 1, 1, false, false>;                     //   debug physics (resets: the noise unit's; no parity replay)
extern template StepLaunch launch_step<kModeActuator | kModeContacts | kModeTerms | 0, 1, false, true, true>;   // orr_kernels_actuator.hip: env step with torque limits + actuator outputs,
extern template StepLaunch launch_step<kModeActuator | kModeTerms | 2, 1, false, true, true>;                   //   its parity replay (resets: the noise unit's; no debug physics)
extern template StepLaunch launch_step<kModeSensor | kModeActuator | kModeContacts | kModeTerms | 0, 1, false, true, true>;   // orr_kernels_sensor.hip: env step with sensor noise,
extern template StepLaunch launch_step<kModeSensor | kModeActuator | kModeTerms | 2, 1, false, true, true>;                   //   its parity replay,
extern template ResetLaunch launch_sensor_reset<true>;
extern template StepLaunch launch_step<kModeRandomizer | kModeSensor | kModeActuator | kModeContacts | kModeTerms | 0, 1, false, true, true>;   // orr_kernels_randomizer.hip: env step with the table-driven randomiser,
extern template StepLaunch launch_step<kModeRandomizer | kModeSensor | kModeActuator | kModeTerms | 2, 1, false, true, true>;                   //   its parity replay,
extern template StepLaunch launch_step<kModePush | kModeRandomizer | kModeSensor | kModeActuator | kModeContacts | kModeTerms | 0, 1, false, true, true>;   // orr_kernels_push.hip: env step with pushes (replays and resets: the randomiser unit's)
extern template ResetLaunch launch_randomizer_reset<true>;                                                                                     //   reset (and its parity replay)                                                                       //   reset (and its parity replay)

// The privileged observation (orr_privileged_obs): no template and no variants, one kernel in a unit of its own with the plain flags
// (orr_kernels_priv.hip).  lat_div = (ORR_RING_DEPTH - 2) * sim_dt, step_dt = action_repeat * sim_dt, formed by the caller
hipError_t launch_privileged_obs(const DevTables* tab, const float* state, int n, const uint8_t* done, float* priv, float lat_div, float step_dt,
                                 hipStream_t stream);

// The shaped reward (orr_shaped_reward) and the setter of its weights (orr_set_reward_shaping): likewise one kernel each in a unit of their
// own with the plain flags (orr_kernels_shaping.hip).  inv_nsub = 1 / action_repeat, inv_dt = 1 / sim_dt, formed by the caller in float32
hipError_t launch_shaped_reward(const DevTables* tab, const float* state, int n, const float* actions, const float* reward_in, const uint8_t* done,
                                float* reward_out, float inv_nsub, float inv_dt, hipStream_t stream);
hipError_t launch_set_shaping(DevTables* tab, const orr_reward_shaping& s, hipStream_t stream);

#ifdef ORR_STAGE_DUMP
// the stage dump: instantiated in BOTH step units (orr_kernels.hip: WPE 1, orr_kernels_w2.hip: WPE 2), which compile different forms of
// the very functions it calls (kCarrySubtreeMass, kOwnLegFactor, their flags)
using StageDumpLaunch = hipError_t(const KParams& P, int waves, hipStream_t stream, const float* torques, float* out, long long out_words);
template <bool ANCHOR, int WPE>
hipError_t launch_stage_dump(const KParams& P, int waves, hipStream_t stream, const float* torques, float* out, long long out_words) {
  hipLaunchKernelGGL((orr_stage_dump_kernel<ANCHOR, WPE>), dim3(waves), dim3(64), 0, stream, P, torques, out, out_words);
  return hipGetLastError();
}
#ifndef ORR_TU_MAIN
extern template StageDumpLaunch launch_stage_dump<false, 1>;                  // orr_kernels.hip
extern template StageDumpLaunch launch_stage_dump<true, 1>;
#endif
#ifndef ORR_TU_STEP_W2
extern template StageDumpLaunch launch_stage_dump<false, 2>;                  // orr_kernels_w2.hip
extern template StageDumpLaunch launch_stage_dump<true, 2>;
#endif
#endif
}  // namespace orr
