// orr_device.h -- device-side building blocks of the quadruped env kernels (gfx950, wave64).
//
// A wavefront serves kRPW = 4 robots, 16 lanes each.
// Lane roles inside a robot's lane group change phase by phase:
//   motors      lanes 0..11   action filter / interpolation / clip / PD torque (minitaur.py:280-293,438-460,706-769)
//   legs        leg = lane & 3, link = lane >> 2: forward dynamics of the 3-link leg chains (pybullet stepSimulation)
//   rows        lanes 0..15   constraint rows in two banks: impulse response, Delassus column, PGS state
//   dofs        18 generalised velocities u = [omega_w, v_w, joint rates]: lane l owns DOF l (lanes 0, 1 also 16, 17)
// Cross-lane data goes through DPP (a robot's 16 lanes are one DPP row) or LDS; register arrays are never indexed
// dynamically.
//
// Arithmetic: float32.  Reference citations are relative to /root/reference/OpenRoboRL/.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/openroborl_hip.h"

#define ORR_PI_F 3.14159265358979323846f
// A workgroup is exactly one wavefront.  A wave's LDS instructions execute in issue order, so a ds_write followed
// by another lane's ds_read of the same word needs no s_waitcnt and no s_barrier -- only the COMPILER must not move
// memory operations across the hand-off.  (A workgroup-scope release/acquire fence also works but makes the wave
// drain vmcnt, i.e. wait for the latency-ring store to reach memory, ten times per sub-step.)
#define WSYNC()                             \
  do {                                      \
    asm volatile("" ::: "memory");          \
    __builtin_amdgcn_wave_barrier();        \
    asm volatile("" ::: "memory");          \
  } while (0)

namespace orr {

constexpr int kLanes = 16;        // lanes of a wavefront that serve one robot: one DPP row
constexpr int kRPW = 64 / kLanes;  // robots per wavefront
constexpr int kMaxRows = 28;  // 4 knee-friction + <=12 joint-limit + 12 contact rows
constexpr int kHead = 308;    // words of the state record staged in LDS: everything before the ring (307) + one spare word (the non-finite guard's flag)

// Clip header (16 words: one per lane when it is staged into LDS).  Times are DOUBLES: the motion time reaches 20 s by the end of a
// 600-step episode, where float32 resolves 2e-6 s = 1e-4 of a frame, and the frame velocities jump by O(10) between frames
// (tests/test_gpu_clips.py).  The sampler runs twice per env step, so its few dozen f64 instructions are free.  dt_d / sim_dt_d
// are the DECIMAL constants of the clip file / yaml (0.01667, 0.001), recovered from the float32 ABI values on the host (dec7).
struct DevClip {
  const float* frames;
  const float* vels;
  int F, flags;
  double dt_d, dur_d;   // FrameDuration, FrameDuration * (F - 1): motion_data.py:198-208
  double sim_dt_d;      // cfg.sim_dt (the same for every clip; kept here because the clip header is what the sampler has in LDS)
  float cdp[3];
  float cdh;
};
static_assert(sizeof(DevClip) == 64, "clip header = 16 words");

// Compact, kernel-facing robot model; built on the host by orr_set_model from orr_model.
// All joints are required to turn about coordinate axes of the kinematic frame: the hip (k = 0) about
// +-x, upper and lower leg (k = 1, 2) about +-y.  The sign is folded into the internal joint angle
//   a = jdir * (q_urdf - joff),  jdir = JOINT_DIRECTION * axis_sign,
// so that inside the kernels every joint turns about +x or +y.
// HOT part: staged in LDS per robot (512 B) - what the 33 sub-steps and the reward's forward kinematics read again and again.
struct ModelHot {
  float jdir[12], joff[12];   // per JOINT (URDF order)
  float joint_lo[12], joint_hi[12];  // limits of the internal angle
  float joint_pos[12][3];
  float toe_pos[4][3];
  float shank_pos[4][3];      // second contact sphere of the lower leg (see orr_model)
  float lower_com[4][3];
  float init_quat[4];
  float toe_radius, shank_radius;
  // toe contact normal row (orr_model::contact_stiffness / contact_damping, folded on the host): constraint-force mixing added to the
  // row's diagonal (0 = rigid) and erp / dt of a penetrating toe contact (rigid: cfg.contact_erp / dt)
  float contact_cfm, contact_erp_dt;
};
static_assert(sizeof(ModelHot) == 512, "LDS budget: 4 robots per wave, two waves per SIMD = 20 KB per wave (DESIGN.md section 3)");
// COLD part: read straight from the device table (global memory, L2-resident) where it is needed - per-motor and per-link constants
// that go into registers once per launch, reset-only data, and the termination-only fall proxies (fetched at the top of the last
// sub-step of an env step).  Round 2 staged all of it in LDS (1420 B per robot), which capped a CU at 5-6 resident waves.
struct ModelCold {
  float init_pos[3];
  float foot_friction;
  float init_motor_angles[12], motor_dir[12], motor_offset[12];
  int joint_of_motor[12];
  float kp[12], kd[12];
  float tau_sign[12];         // per joint: internal torque = tau_sign * motor torque
  float tau_sign_motor[12];   // the same per MOTOR (tau_sign[joint_of_motor[m]]): no dependent second load
  float link_com[12][3];
  float default_joints[12];   // (INIT_MOTOR_ANGLES + OFFSET) * DIR, motor order (imitation_task.py:1245-1252)
  int num_fall;
  int fall_body[ORR_MAX_FALL_PROXIES];
  float fall_pos[ORR_MAX_FALL_PROXIES][3];
  float fall_radius[ORR_MAX_FALL_PROXIES];
  // mass properties before randomisation: body 0 = base, 1 + j = link j
  float mass[13];
  float inertia[13][6];
  float inertia_pa[13][6];
  int group[13];
  int friction_anchor;        // orr_model::friction_anchor (read by the anchor variant of the step kernel only; LAST: the fields above keep their offsets)
};
struct alignas(16) DevModel {   // 16-byte aligned in the device table: the hot part is copied to LDS in 16-byte pieces
  ModelHot hot;
  ModelCold cold;
};
static_assert(sizeof(DevModel) % 16 == 0 && offsetof(DevModel, hot) == 0, "16-byte pieces");
constexpr int kModelLdsWords = (int)(sizeof(ModelHot) / 4);

struct DevTables {
  DevModel model[ORR_MAX_ROBOT_TYPES];
  DevClip clip[ORR_MAX_CLIPS];
  // clip sets (orr_set_clip_set): read by the multi-clip variants of the kernels only (orr_kernels_multiclip.hip).  APPENDED: the fields
  // above keep their offsets, so the default kernels see the table they always saw
  int clip_set[ORR_MAX_ROBOT_TYPES][ORR_MAX_CLIPS];   // a type's set = 64 bytes, one word per lane of a robot
  int clip_set_n[ORR_MAX_ROBOT_TYPES];                // 0 = no set: a reset keeps the record's CLIP_ID
  int* clip_log;                                      // orr_bind_clip_log: clip of each logged episode (row = episode-log slot), or NULL
  // mid-episode clip switching (orr_set_clip_switch), read by the multi-clip variants only.  APPENDED like the clip sets
  float clip_switch[ORR_MAX_ROBOT_TYPES][2];          // (tmin, tmax) of a type's switch interval; (+inf, +inf) = never
  // task noise of the handle (orr_set_task_noise), read by the noise variants only (orr_kernels_noise.hip).  APPENDED likewise
  orr_task_noise noise;                               // all zero = off
  // per-term reward outputs (orr_bind_reward_terms), read by the terms variant only (orr_kernels_terms.hip).  APPENDED likewise
  float* terms;                                       // [N][5] the unweighted terms of the step's reward, or NULL = not bound
  float* term_sums;                                   // [N][5] their running sums over the robot's current episode
  float* term_log;                                    // [ep_log_capacity][5] sums of each logged episode (row = episode-log slot), or NULL
  // foot contact outputs (orr_bind_contact_outputs), read by the contact variants only (orr_kernels_contacts.hip).  APPENDED likewise
  float* contact_out;                                 // [N][16] per leg: sums of the launch's normal / friction x / friction y impulses, largest normal impulse; NULL = not bound
  float* contact_ep;                                  // [N][8] per leg: stance steps and sum of the normal sums over the robot's current episode
  float* contact_log;                                 // [ep_log_capacity][8] contact_ep row of each logged episode (row = episode-log slot), or NULL
  // motor torque limits and actuator outputs (orr_set_torque_limits, orr_bind_actuator_outputs), read by the actuator variants only
  // (orr_kernels_actuator.hip).  APPENDED likewise
  float* act_out;                                     // [N][12][4] per motor: sum tau, max |tau|, sum tau^2, work over the launch's sub-steps; NULL = not bound
  float* act_ep;                                      // [N][4] work, sum tau^2, largest |tau|, saturated steps over the robot's current episode
  float* act_log;                                     // [ep_log_capacity][4] act_ep row of each logged episode (row = episode-log slot), or NULL
  float torque_limit[ORR_MAX_ROBOT_TYPES][12];        // per motor, N m, on the strength-scaled PD torque; +inf = none (orr_create fills the table with it)
  // sensor noise of the handle (orr_set_sensor_noise), read by the sensor variants only (orr_kernels_sensor.hip).  APPENDED likewise
  orr_sensor_noise sensor;                            // all zero = off; motor_velocity_std / motor_torque_std have no consumer
  // domain randomisation of the handle (orr_set_randomizer, orr_bind_randomizer_params), read by the randomiser variants only
  // (orr_kernels_randomizer.hip).  APPENDED likewise
  orr_randomizer rnd;                                 // orr_create fills in the built-in six ranges
  float* rand_params;                                 // [N][ORR_RAND_ROW] the episode's normalised samples per robot, or NULL = not bound
  int rand_suspend;                                   // != 0: resets apply the rows instead of drawing, and do not write them
  // external pushes of the handle (orr_set_push, orr_bind_push_outputs), read by the push variant only (orr_kernels_push.hip).
  // APPENDED likewise
  orr_push push;                                      // all zero = off
  float* push_out;                                    // [N][ORR_PUSH_ROW] dv, dw, kicked, kicks of the episode per robot, or NULL = not bound
  int push_table;                                     // != 0: the handle has a randomiser table or params buffer, so the push variant's auto-reset is the table-driven one; 0: the built-in literal ranges, as in the kernels below the randomiser variants
  // weighted clip draws (orr_set_clip_set writes the uniform thresholds, orr_set_clip_weights others), read by the multi-clip variants
  // only; the clip curriculum's kernel (orr_clip_curriculum_update) WRITES them, so the device's copy is the truth: past orr_create
  // nothing copies the host's mirror of these two members over it.  APPENDED likewise
  unsigned int clip_cum[ORR_MAX_ROBOT_TYPES][ORR_MAX_CLIPS + 1];   // 24-bit-scale thresholds: entry k is drawn iff cum[k] <= m < cum[k + 1]; cum[0] = 0, cum[n] = 2^24
  struct ClipCurriculum {
    float alpha, eps;                                 // orr_clip_curriculum's settings
    int metric;
    float ref[ORR_MAX_CLIPS];
    double ema[ORR_MAX_CLIPS];                        // per clip id: the running score in [0, 1]; the kernel's own state
  } cur;
  // reward shaping of the handle (orr_set_reward_shaping, orr_bind_reward_shaping), read by orr_shaped_reward's kernel only
  // (orr_kernels_shaping.hip), which follows the step and is no variant of it.  APPENDED likewise
  float* shape_out;                                   // [N][ORR_SHAPING_ROW] the step's six unweighted terms, the shaped reward, 1.0; NULL = not bound
  float* shape_ep;                                    // [N][ORR_SHAPING_ROW] their sums over the robot's current episode
  float* shape_tot;                                   // [N][ORR_SHAPING_ROW] the sums of the robot's finished episodes
  float* shape_prev;                                  // [N][24] the robot's last two actions, the newer first
  orr_reward_shaping shaping;                         // the weights and the floor; its kernel's setter writes the device's copy in stream order
};
// Flag bit of orr_step_kernel's MODE: the variant that also writes the reward terms.  MODE & 3 is the mode proper (0 env step, 1 debug
// physics, 2 parity replay).  A bit of MODE rather than a template parameter of its own: the older variants keep their mangled names
constexpr int kModeTerms = 4;
// Likewise: the variant that also sums the sub-steps' foot contact impulses (orr_bind_contact_outputs).  Env step and debug physics only
constexpr int kModeContacts = 8;
// Likewise: the variant that clips the sub-steps' motor torques to the type's limits and keeps per-motor torque / work accumulators
// (orr_set_torque_limits, orr_bind_actuator_outputs).  Env step and parity replay only: orr_debug_physics takes its torques as given
constexpr int kModeActuator = 16;
// Likewise: the variant whose sensor readings carry Gaussian noise (orr_set_sensor_noise).  Env step and parity replay, on top of the
// actuator variants
constexpr int kModeSensor = 32;
// Likewise: the variant whose auto-reset runs the table-driven randomiser (orr_set_randomizer, orr_bind_randomizer_params).  Env step and
// parity replay, on top of the sensor variants
constexpr int kModeRandomizer = 64;
static_assert(sizeof(orr_randomizer) == 12 * ORR_RAND_NUM_PARAMS && ORR_RAND_NUM_PARAMS == 10 && ORR_RAND_ROW == 32,
              "the randomiser variants read it as three tables of ten words; a row is two words per lane");
// What the caller of reset_robot_state<.., RAND> hands in and gets back.  row: the robot's row of the params buffer (NULL = not bound),
// suspend: apply the row instead of drawing.  a, b: the lane's two words of the new episode's row (words lane and 16 + lane), which the
// caller stores at the end of its kernel, behind every load (store_rand_row)
// Likewise: the variant that kicks the robot's base twist at the start of the step (orr_set_push, orr_bind_push_outputs).  Env step only,
// on top of the randomiser variant
constexpr int kModePush = 128;
static_assert(sizeof(orr_push) == 24 && ORR_PUSH_ROW == 8, "the push variant reads it as six words; a row is one word per lane 0..7");
// The handle's push settings, wave-uniform (one setting per handle), and the outputs buffer (NULL = not bound).  span = lin_hi - lin_lo
struct PushSet {
  float prob = 0.0f, lin_lo = 0.0f, span = 0.0f, lin_z = 0.0f, ang = 0.0f;
  int grace = 0;
  float* out = nullptr;
  bool table = false;   // the auto-reset runs the table-driven randomiser (DevTables::push_table)
};
struct RandRow {
  const float* row = nullptr;
  bool suspend = false;
  float a = 0.0f, b = 0.0f;
};
static_assert(sizeof(orr_sensor_noise) == 20, "the sensor variants read it as five words");
// The three deviations of orr_sensor_noise that have a consumer, wave-uniform (one setting per handle): motor angle, base rpy, base rpy
// rate.  All zero in every variant but the sensor ones, whose code for them is compiled out
struct SensorNoise {
  float a = 0.0f, r = 0.0f, d = 0.0f;
};
static_assert(sizeof(orr_task_noise) == 32, "the noise variants read it as eight words");

// Replay inputs of the parity entry points orr_debug_replay_reset / orr_debug_replay_step (kernel MODE 2): the scripted states,
// link positions, contact flags and random draws recorded while the reference's own Python was driven with a scripted pybullet
// client (tests/golden/make_golden_task.py).  All NULL in the product launches.
struct ReplayArgs {
  const float* traj;       // [N][action_repeat][37] rigid state after each sub-step: replaces physics_substep
  const float* eff;        // [N][2][8][3] link positions for the end-effector reward: [0] sim robot, [1] reference model
  const uint8_t* fall;     // [N] a ground contact on a non-foot link was reported
  float* tau_out;          // [N][action_repeat][12] motor torques of the actuator chain (motor order), recorded
  const float* uniforms;   // [N][28] random draws in [0, 1): replace the Philox stream at reset
};

struct KParams {
  orr_config cfg;
  float fb[3], fa[3];  // Butterworth coefficients (action_filter.py:196-217), computed on the host in double
  const DevTables* tab;
  float* state;
  long long* counters;
  float* ep_log;
  int ep_log_cap;
  int simds;           // SIMDs of the device: workgroup b belongs to dispatch round b / simds (two-waves-per-SIMD variant: priority alternation)
  int anchor_on;       // some robot type has orr_model::friction_anchor: the launches run the anchor variant of the step kernel, resets clear the anchors
#ifdef ORR_WAVE_TIMELINE
  long long* wave_times;   // development aid (orr_debug_wave_times): 4 words per wave of the step kernel, every variant
  int wave_times_cap;      // waves it has room for (0 until it is allocated)
#endif
};
// The cold part of a robot type's model, as a GLOBAL-address-space pointer: loads through it are global_load instructions (a generic
// pointer would make them FLAT loads, which also count on the LDS counter and serialise with every LDS access in between).
typedef const ModelCold __attribute__((address_space(1)))* ColdPtr;
__device__ __forceinline__ ColdPtr model_cold(const KParams& P, int robot_type) { return (ColdPtr)&P.tab->model[robot_type].cold; }

// ------------------------------------------------------------------------------------------------
// LDS image of one robot: ~6.6 KB, four per wave
// ------------------------------------------------------------------------------------------------
// The LDS structures are 16-byte aligned and sized in multiples of 16 bytes so that runs of consecutive words are moved
// with ds_read_b128 / ds_write_b128 (a quarter of the LDS instructions of the 4-byte-aligned layout).
struct alignas(16) LinkCache {  // per movable link, written by the lane that owns the link (leg, part), read by the row lanes
  float Rw[9];      // link -> world
  float ow[3];      // link origin, world
  float s[3], sv[3];  // motion axis of the joint in front of the link, about the base COM: (axis; (origin - base) x axis)
};
// Index 3 of the per-part arrays below (and lc[12..15], W[kMaxRows], ustar[18..21]) are DUMP slots for the lanes that own no link /
// joint / row: every lane then stores unconditionally -- a divergent `if` costs a lone wave 20-35 ticks (profiles/r02_issue_costs.txt).
struct alignas(16) LegExchange {  // per leg, hand-over between the lanes (parts) of a leg inside leg_dynamics
  float F[4][6];      // F_k = Ic_k S_k of joint k, written by part k
  float Hc[4][4];     // Hc[k][i] = S_i . F_k (valid for i <= k)
  float b[4];         // tau_k - C_k
};
struct alignas(16) LegSolve {   // per leg: column k of T written by the leg's part-k lane, Hi by all of them; read by the row lanes
  float T[3][6];    // F H^-1: column k = base wrench (angular; linear, world axes, about the base COM) per unit of joint k
  float Hi[6];      // H^-1 of the leg's 3x3 joint-space inertia (00 11 22 01 02 12)
};
static_assert(sizeof(LegSolve) == 96, "LDS budget");

// Code alignment of the hand-written loops.  A lone wave pays for instruction fetch: an 8-byte instruction (VOP3, DPP) that starts on an
// odd dword costs ~0.7 ticks more than an aligned one (shifting the whole kernel by one dword changes its run time by 2.5 %; DESIGN.md
// section 6), and the Gauss-Seidel loops are almost entirely 8-byte instructions with a few 4-byte ones in between -- with the wrong
// start parity 45 of the 57 eight-byte instructions of a sweep are misaligned, with the right one 11.  Left alone, that parity is decided
// by whatever code happens to precede the loop.  The loops therefore align themselves to 8 bytes and add one 4-byte s_nop if their bit of
// ORR_PARITY is set (bit 12: sweeps without the joint-limit bank, bit 13: with it); chosen on the GPU (tools/parity_search.py:
// bit 12 = 0.244 ms, clear = 0.249 ms; bit 13 and the parity of the compiler-generated phases make no measurable difference).
#ifndef ORR_PARITY
#define ORR_PARITY 0x1000
#endif
#define ORR_STR2(x) #x
#define ORR_STR(x) ORR_STR2(x)
constexpr int kPhaseSlots = 40;   // phase timers of the -DORR_PHASE_TIMERS build (tools/phase_cycles.py)
constexpr int kWStride = 20;   // 18 DOFs, padded to a multiple of 16 bytes
struct alignas(16) DynamicsBuf {           // leg dynamics -> row setup hand-over (dead once the impulse responses are written)
  LinkCache lc[16];           // 12 links + the part-3 lanes' dump slots
  LegExchange legx[4];
};
union alignas(16) SubstepBuf {            // live only inside a physics sub-step
  float W[kMaxRows + 1][kWStride];  // M^-1 J^T per row slot (18 used): written by the impulse responses, read until the velocity update
  DynamicsBuf dyn;            // shares its space: written by the next sub-step's dynamics, last read by the row setup
};
struct alignas(16) StepEndBuf {           // live only at reset / end of step
  union {
    struct {
      float frames[11][19];   // staged clip frames: 5 sample times x (f0, f1) + frame 0
      float fvel[2][18];
    };
    // the observation being assembled shares the space of the staged frames: it is written (build_obs: once per robot, at the end of
    // the step and behind an inline reset, or at the end of the reset kernel) only after the frames were blended into pose[] / vel[]
    // (sample_poses_finish)
    float obs[ORR_OBS_DIM];
  };
  float pose[5][19];          // sampled reference poses (update time + 4 target times)
  float vel[18];
  float ee[2][8][3];          // end-effector world positions, [0] sim [1] ref
  float red[80];              // small cross-lane reductions of the step-end code; reset_robot_state: ring entries #1 / #2 and the 28 draws
};
static_assert(sizeof(StepEndBuf) <= sizeof(SubstepBuf), "LDS budget: the step-end buffers fit into the sub-step buffers' space");
union PhaseBuf {
  SubstepBuf sub;
  StepEndBuf end;
};

struct alignas(16) Shared {
  alignas(16) float s[kHead];  // state head (float / int bit patterns)
  alignas(16) ModelHot m;      // robot model (hot part)
  alignas(16) DevClip clip;    // header of the robot's motion clip (copied once per launch: its fields are read many times at the end of a step)
  LegSolve leg[4];
  alignas(16) float tdump[8];  // where the part-3 lanes (which own no joint) put their "column of T" (leg_dynamics)
  alignas(16) float Rb[9];     // kinematic base frame -> world
  alignas(16) float tau[16];   // joint torques (internal sign convention), joint order; 12..15: dump slots of the lanes that own no motor
  alignas(16) float ustar[24];
  alignas(16) float co[20];    // control (latency-delayed) observation
  alignas(16) PhaseBuf ph;
#ifdef ORR_PHASE_TIMERS
  long long pt_acc[kPhaseSlots], pt_last;  // development aid, see PT() in orr_env_kernels.h
#endif
};

// ------------------------------------------------------------------------------------------------
// small math (xyzw quaternions; pose3d.py / pybullet_utils.transformations semantics)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cross3(const float a[3], const float b[3], float o[3]) {
  float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  o[0] = x; o[1] = y; o[2] = z;
}
__device__ __forceinline__ void mv3(const float M[9], const float v[3], float o[3]) {
  float a = M[0] * v[0] + M[1] * v[1] + M[2] * v[2];
  float b = M[3] * v[0] + M[4] * v[1] + M[5] * v[2];
  float c = M[6] * v[0] + M[7] * v[1] + M[8] * v[2];
  o[0] = a; o[1] = b; o[2] = c;
}
__device__ __forceinline__ void mtv3(const float M[9], const float v[3], float o[3]) {
  float a = M[0] * v[0] + M[3] * v[1] + M[6] * v[2];
  float b = M[1] * v[0] + M[4] * v[1] + M[7] * v[2];
  float c = M[2] * v[0] + M[5] * v[1] + M[8] * v[2];
  o[0] = a; o[1] = b; o[2] = c;
}
__device__ __forceinline__ void symv(const float S[6], const float v[3], float o[3]) {
  const float a = S[0] * v[0] + S[3] * v[1] + S[4] * v[2];
  const float b = S[3] * v[0] + S[1] * v[1] + S[5] * v[2];
  const float c = S[4] * v[0] + S[5] * v[1] + S[2] * v[2];
  o[0] = a; o[1] = b; o[2] = c;
}

// sum of x over the 16 lanes of this robot (one DPP row), in every lane: quad butterflies, then the two mirror permutes
__device__ __forceinline__ float row_sum16(float x) {
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true));   // quad_perm:[1,0,3,2]
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, true));   // quad_perm:[2,3,0,1]
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xF, 0xF, true));  // row_half_mirror
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x140, 0xF, 0xF, true));  // row_mirror
  return x;
}

// largest x over the 16 lanes of this robot, in every lane: the same four steps
__device__ __forceinline__ float row_max16(float x) {
  x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true)));   // quad_perm:[1,0,3,2]
  x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, true)));   // quad_perm:[2,3,0,1]
  x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xF, 0xF, true)));  // row_half_mirror
  x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x140, 0xF, 0xF, true)));  // row_mirror
  return x;
}

// value of x in lane R (< 16) of this robot's lane group.  With 16 lanes per robot a robot is one DPP row and the
// broadcast is a single v_mov_b32_dpp row_newbcast:R (gfx90a+; every lane of the wave is active at the call sites).
template <int R>
__device__ __forceinline__ float bcast_lane(float x, int sub) {
  const int v = __float_as_int(x);
  // old = 0 with bound_ctrl (every source lane of a row_newbcast is valid, so neither matters): the form the compiler's DPP
  // combiner folds into the consuming VOP2 (v_mul_f32_dpp / v_fmac_f32_dpp / v_max_f32_dpp ...) instead of a separate v_mov_b32_dpp
  return __int_as_float(__builtin_amdgcn_update_dpp(0, v, 0x150 + R, 0xF, 0xF, true));
}
// The three Delassus entries of one leg's contact rows (normal z, friction x, friction y) for the impulse response (wa, wq) held
// by this lane: t = wa_lin + wa_ang x rr + sum_k ck[k] wq[k], where rr (contact point relative to the base COM) and ck[k]
// (velocity of the contact point per unit rate of joint k of that leg) come from lane R (the leg's normal-row lane) as DPP
// operands.  18 instructions for three columns (three separate 9-term dot products: 30).
template <int R>
__device__ __forceinline__ void dpp_contact_triplet(float rr0, float rr1, float rr2, float c00, float c01, float c02, float c10, float c11,
                                                    float c12, float c20, float c21, float c22, float wa0, float wa1, float wa2, float wa3,
                                                    float wa4, float wa5, float q0, float q1, float q2, float& tx, float& ty, float& tz) {
  static_assert(kRPW == 4, "row_newbcast needs 16 lanes per robot");
#define ORR_NB " row_newbcast:%21 row_mask:0xf bank_mask:0xf\n\t"
  asm("s_nop 1\n\t"
      "v_mul_f32_dpp %0, %5, %16" ORR_NB     // tx  = rr2 * wa1
      "v_mul_f32_dpp %1, %3, %17" ORR_NB     // ty  = rr0 * wa2
      "v_mul_f32_dpp %2, %4, %15" ORR_NB     // tz  = rr1 * wa0
      "v_fmac_f32_dpp %0, -%4, %17" ORR_NB   // tx -= rr1 * wa2
      "v_fmac_f32_dpp %1, -%5, %15" ORR_NB   // ty -= rr2 * wa0
      "v_fmac_f32_dpp %2, -%3, %16" ORR_NB   // tz -= rr0 * wa1
      "v_add_f32 %0, %0, %18\n\t"
      "v_add_f32 %1, %1, %19\n\t"
      "v_add_f32 %2, %2, %20\n\t"
      "v_fmac_f32_dpp %0, %6, %22" ORR_NB
      "v_fmac_f32_dpp %1, %7, %22" ORR_NB
      "v_fmac_f32_dpp %2, %8, %22" ORR_NB
      "v_fmac_f32_dpp %0, %9, %23" ORR_NB
      "v_fmac_f32_dpp %1, %10, %23" ORR_NB
      "v_fmac_f32_dpp %2, %11, %23" ORR_NB
      "v_fmac_f32_dpp %0, %12, %24" ORR_NB
      "v_fmac_f32_dpp %1, %13, %24" ORR_NB
      "v_fmac_f32_dpp %2, %14, %24 row_newbcast:%21 row_mask:0xf bank_mask:0xf"
      : "=&v"(tx), "=&v"(ty), "=&v"(tz)
      : "v"(rr0), "v"(rr1), "v"(rr2),                                             // 3 4 5
        "v"(c00), "v"(c01), "v"(c02), "v"(c10), "v"(c11), "v"(c12),               // 6..11
        "v"(c20), "v"(c21), "v"(c22),                                             // 12 13 14
        "v"(wa0), "v"(wa1), "v"(wa2), "v"(wa3), "v"(wa4), "v"(wa5),               // 15..20
        "n"(R), "v"(q0), "v"(q1), "v"(q2));                                       // 21, 22 23 24
#undef ORR_NB
}
// max(x in lane R of this robot, 0) in one instruction (v_max_f32_dpp): the clamp of a unilateral row (contact normal, joint
// limit: bounds [0, inf)) fused with its broadcast.  x has usually just been written, hence the s_nop (DPP read hazard).
template <int R>
__device__ __forceinline__ float dpp_bcast_max0(float x, float zero) {
  static_assert(kRPW == 4, "row_newbcast needs 16 lanes per robot");
  float o;
  asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "=v"(o) : "v"(x), "v"(zero), "n"(R));
  return o;
}

// sine / cosine of a joint angle (|a| is a few radians at most).  Cody-Waite reduction to [-pi/4, pi/4] with a
// two-part pi/2 and minimax polynomials (~25 instructions, no approximate hardware instruction; error < 1e-7 for |a| <= 100,
// measured on the device: tests/test_gpu_device_primitives.py, profiles/device_primitives.txt; no large-argument branch): +2.3 % env steps/s
// over libm's sincosf at unchanged parity tolerances.
__device__ __forceinline__ void joint_sincos(float a, float* sn, float* cs) {
  const float k = rintf(a * 0.63661977236758134f);       // a * 2/pi
  float r = fmaf(-k, 1.57079625129699707031f, a);         // pi/2 high part (exact in float)
  r = fmaf(-k, 7.54978941586159635335e-08f, r);           // pi/2 low part
  const float r2 = r * r;
  // sin(r), |r| <= pi/4
  float ps = fmaf(r2, -1.9515295891e-4f, 8.3321608736e-3f);
  ps = fmaf(ps, r2, -1.6666654611e-1f);
  const float s = fmaf(ps * r2, r, r);
  // cos(r)
  float pc = fmaf(r2, 2.443315711809948e-5f, -1.388731625493765e-3f);
  pc = fmaf(pc, r2, 4.166664568298827e-2f);
  const float c = fmaf(pc * r2, r2, fmaf(r2, -0.5f, 1.0f));
  const int q = (int)k & 3;
  const float ss = (q & 1) ? c : s, cc = (q & 1) ? s : c;
  *sn = (q & 2) ? -ss : ss;
  *cs = ((q + 1) & 2) ? -cc : cc;
}

// Inverse trigonometric functions without branches (libm's atan2f / asinf / acosf cost a lone wave several taken or skipped
// branches each, 13-30 ticks apiece: profiles/r02_issue_costs.txt).  atan2: octant reduction to t = min / max in [0, 1], then the
// Cephes atanf kernel on [0, tan(pi/8)] (t -> (t - 1) / (t + 1) above it); absolute error < 3e-7 with a correctly rounded
// reciprocal (float64 check on 2 M random arguments); the device's 1-ulp v_rcp_f32 is on the path once, twice above the switch, and adds up
// to 1.2e-7: the tested bound is 4.2e-7 over magnitudes 4.7e-38 .. 1e30 (tests/test_gpu_device_primitives.py; the measured maximum is
// in profiles/device_primitives.txt).  asin_bf and everything built on these inherit both figures.
// NaN arguments come out FINITE (fmax / fmin and the selects drop NaNs): non-finite numbers
// are detected in ONE place, the |state| < 1e30 sweep + reward check at the end of the step (ORR_DONE_NAN, orr_env_kernels.h), never through
// these functions (tests/test_gpu_parity.py::test_non_finite_state_is_caught_by_the_state_guard).
__device__ __forceinline__ float atan2_bf(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  // v_rcp_f32 takes a subnormal argument for zero (-> +inf; 0 * inf = NaN, and a subnormal mn gives inf, then NaN in the (t - 1) / (t + 1)
  // branch): arguments below 2^-63 are scaled by 2^64 first, both alike, which is exact (tests/test_gpu_device_primitives.py).  This
  // relies on the env units keeping float32 denormals (the compiler's default for gfx950, .amdhsa_float_denorm_mode_32 3): were they
  // flushed (-fgpu-flush-denormals-to-zero), mx * sc would be 0 again and the NaN back.  Four instructions per call, asin_bf included.
  const float sc = mx < 1.0842022e-19f ? 1.8446744e19f : 1.0f;
  const float t = mx > 0.0f ? (mn * sc) * __builtin_amdgcn_rcpf(mx * sc) : 0.0f;
  const bool big = t > 0.41421356237f;
  const float u = big ? (t - 1.0f) * __builtin_amdgcn_rcpf(t + 1.0f) : t;
  const float z = u * u;
  float p = fmaf(z, 8.05374449538e-2f, -1.38776856032e-1f);
  p = fmaf(p, z, 1.99777106478e-1f);
  p = fmaf(p, z, -3.33329491539e-1f);
  float r = fmaf(p * z, u, u);
  r = big ? r + 0.78539816339744831f : r;
  r = ay > ax ? 1.57079632679489662f - r : r;
  // quadrant by the SIGN BITS, like libm: atan2(0, -0.0) = pi and atan2(-0.0, -1) = -pi (a comparison with 0.0f treats -0.0 as positive)
  r = __float_as_int(x) < 0 ? 3.14159265358979324f - r : r;
  return __float_as_int(y) < 0 ? -r : r;
}
__device__ __forceinline__ float asin_bf(float x) {   // |x| <= 1
  return atan2_bf(x, __builtin_amdgcn_sqrtf(fmaxf((1.0f - x) * (1.0f + x), 0.0f)));
}

// transformations.quaternion_multiply(a, b): Hamilton product (pose3d.py:228-230)
__device__ __forceinline__ void qmul(const float a[4], const float b[4], float o[4]) {
  float x1 = a[0], y1 = a[1], z1 = a[2], w1 = a[3], x0 = b[0], y0 = b[1], z0 = b[2], w0 = b[3];
  o[0] = x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0;
  o[1] = -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0;
  o[2] = x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0;
  o[3] = -x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0;
}
__device__ __forceinline__ void qconj(const float q[4], float o[4]) { o[0] = -q[0]; o[1] = -q[1]; o[2] = -q[2]; o[3] = q[3]; }
__device__ __forceinline__ void qinv(const float q[4], float o[4]) {
  float n = __builtin_amdgcn_rcpf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  o[0] = -q[0] * n; o[1] = -q[1] * n; o[2] = -q[2] * n; o[3] = q[3] * n;
}
// pose3d.QuaternionRotatePoint (pose3d.py:213-231): q [p,0] q^-1
__device__ __forceinline__ void qrot(const float p[3], const float q[4], float o[3]) {
  float qp[4] = {p[0], p[1], p[2], 0.0f}, qi[4], t[4], r[4];
  qinv(q, qi);
  qmul(q, qp, t);
  qmul(t, qi, r);
  o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
}
__device__ __forceinline__ void qstd(float q[4]) {  // pose3d.py:289-301
  const float sg = q[3] < 0.0f ? -1.0f : 1.0f;
  q[0] *= sg; q[1] *= sg; q[2] *= sg; q[3] *= sg;
}
__device__ __forceinline__ float qheading(const float q[4]) {  // pose3d.py:325-341
  float x[3] = {1.0f, 0.0f, 0.0f}, r[3];
  qrot(x, q, r);
  return atan2_bf(r[1], r[0]);
}
__device__ __forceinline__ void q_about_z(float ang, float o[4]) {
  float s, c;
  joint_sincos(0.5f * ang, &s, &c);
  o[0] = 0.0f; o[1] = 0.0f; o[2] = s; o[3] = c;
}
// |angle| of pose3d.QuaternionToAxisAngle + normalize_rotation_angle (pose3d.py:139-187,304-322)
__device__ __forceinline__ float q_norm_angle(const float q[4]) {
  const float n = __builtin_amdgcn_sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  const float ang = 2.0f * atan2_bf(n, q[3]);   // in [0, 2 pi] (n >= 0)
  // beyond pi: fmod(ang, 2 pi) (= ang here, or 0 at exactly 2 pi) minus a full turn
  const float m = ang >= 2.0f * ORR_PI_F ? ang - 2.0f * ORR_PI_F : ang;
  return ang > ORR_PI_F ? m - 2.0f * ORR_PI_F : ang;
}
// 1 / sqrt(x) for a normal positive x (sums of squares of unit-ish quaternions, pivots of the base inertia): the bare hardware
// instruction (1 ulp); libm's rsqrtf wraps it in a denormal-range rescaling, five more instructions per call
__device__ __forceinline__ float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
// x[lane & 3] as a two-level select on the bits of the lane (a chain of `lane == k ? ... :` on one variable is turned into a switch by
// the optimiser, which the back end lowers to nested divergent branches: 20-35 ticks each for a lone wave)
__device__ __forceinline__ float pick4(int lane, float x0, float x1, float x2, float x3) {
  const bool b0 = (lane & 1) != 0, b1 = (lane & 2) != 0;
  const float lo = b0 ? x1 : x0, hi = b0 ? x3 : x2;
  return b1 ? hi : lo;
}
__device__ __forceinline__ float map_pi(float a) {  // pose3d.MapToMinusPiToPi (pose3d.py:358-374)
  // fmod(a, 2 pi) without libm's loop and branches (a taken or skipped branch costs a lone wave 3-6 multiply-adds): whole turns
  // k = trunc(a / 2 pi), removed with a two-part 2 pi; exact (k = 0: m = a) for |a| < 2 pi, i.e. for every joint angle;
  // beyond that within one ulp of |a| + 2.4e-7 for |a| <= 1000 (both tested on the device: tests/test_gpu_device_primitives.py)
  const float k = truncf(a * 0.15915494309189535f);
  float m = fmaf(-k, 6.2831854820251465f, a);       // 2 pi rounded to float ...
  m = fmaf(-k, -1.7484555e-07f, m);                 // ... and the rest of it
  m = m >= ORR_PI_F ? m - 2.0f * ORR_PI_F : (m < -ORR_PI_F ? m + 2.0f * ORR_PI_F : m);
  return m;
}
__device__ __forceinline__ void q_to_mat(const float qin[4], float R[9]) {
  float n = rsq(qin[0] * qin[0] + qin[1] * qin[1] + qin[2] * qin[2] + qin[3] * qin[3]);
  float x = qin[0] * n, y = qin[1] * n, z = qin[2] * n, w = qin[3] * n;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
// pybullet.getEulerFromQuaternion: roll, pitch, yaw (Bullet ZYX)
__device__ __forceinline__ void euler_from_quat(const float q[4], float rpy[3]) {
  float x = q[0], y = q[1], z = q[2], w = q[3];
  float sqx = x * x, sqy = y * y, sqz = z * z, sqw = w * w;
  float sarg = -2.0f * (x * z - w * y);
  rpy[0] = atan2_bf(2.0f * (y * z + w * x), -sqx - sqy + sqz + sqw);
  rpy[1] = asin_bf(fminf(fmaxf(sarg, -1.0f), 1.0f));     // = -+ pi / 2 at the clamped ends
  rpy[2] = atan2_bf(2.0f * (x * y + w * z), sqx - sqy - sqz + sqw);
}
// transformations.quaternion_slerp (shortest path)
__device__ __forceinline__ void qslerp(const float a[4], const float b[4], float f, float o[4]) {
  // the reference's "the ends coincide" threshold is 4 x the float64 epsilon on |d| - 1 (and on the angle), i.e. an angle below
  // 4e-8 rad: consecutive frames of the slow clips (inplace_steps, sidesteps: 1e-3 rad apart) ARE interpolated.  In float32 the dot
  // product cannot resolve 1 - |d| = angle^2 / 2 there, so 1 - |d| is taken from the difference quaternion (exact subtraction of
  // nearby values), and the angle and its sine come from the same number: s0 + s1 = 1 + O(angle^2) whatever its rounding
  // (round 2 used float32's epsilon and acos(|d|): up to 5e-4 off on those clips, tests/test_gpu_clips.py)
  const float EPS = 2.220446049250313e-16f * 4.0f;
  float n0 = rsq(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]);
  float n1 = rsq(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
  float q0[4] = {a[0] * n0, a[1] * n0, a[2] * n0, a[3] * n0};
  float q1[4] = {b[0] * n1, b[1] * n1, b[2] * n1, b[3] * n1};
  float d = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3];
  // no branches: the general formula is evaluated always and the special cases of the reference are selected afterwards
  const float sgn = d < 0.0f ? -1.0f : 1.0f;
  const float e0 = q1[0] - sgn * q0[0], e1 = q1[1] - sgn * q0[1], e2 = q1[2] - sgn * q0[2], e3 = q1[3] - sgn * q0[3];
  const float omd = fminf(0.5f * (e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3), 1.0f);        // 1 - |d|
  const float sn = __builtin_amdgcn_sqrtf(fmaxf(omd * (2.0f - omd), 1e-36f));            // sin(angle), angle = acos |d| in [0, pi/2]
  const float ang = atan2_bf(sn, 1.0f - omd);
  float sa, sb, unused;
  joint_sincos((1.0f - f) * ang, &sa, &unused);
  joint_sincos(f * ang, &sb, &unused);
  const float isin = __builtin_amdgcn_rcpf(sn);
  const bool first = f == 0.0f, second = f == 1.0f;
  const bool same = omd < EPS || ang < EPS;   // the ends coincide
  const float s0 = first ? 1.0f : (second ? 0.0f : (same ? 1.0f : sa * isin));
  const float s1 = first ? 0.0f : (second ? 1.0f : (same ? 0.0f : sgn * sb * isin));
#pragma unroll
  for (int i = 0; i < 4; i++) o[i] = q0[i] * s0 + q1[i] * s1;
}

// ------------------------------------------------------------------------------------------------
// Philox4x32-10 (same stream definition as oracle/orr_oracle.c: key = seed, ctr = (robot, episode, idx>>2, "ORRL"))
// ------------------------------------------------------------------------------------------------
// one whole block: draws 4 * block .. 4 * block + 3 of stream (robot, episode)
__device__ __forceinline__ void philox_block(unsigned long long seed, uint32_t robot, uint32_t episode, uint32_t block, float u[4]) {
  uint32_t c0 = robot, c1 = episode, c2 = block, c3 = 0x4F52524Cu;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; r++) {
    uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  u[0] = (float)(c0 >> 8) * (1.0f / 16777216.0f); u[1] = (float)(c1 >> 8) * (1.0f / 16777216.0f);
  u[2] = (float)(c2 >> 8) * (1.0f / 16777216.0f); u[3] = (float)(c3 >> 8) * (1.0f / 16777216.0f);
}

// A pair of standard normals from two of the stream's 24-bit uniforms (ua, ub = m / 2^24, either can be exactly 0): Box-Muller,
//   r = sqrt(-2 ln(1 - ua)),  z0 = r cos(2 pi ub),  z1 = r sin(2 pi ub),
// to |z - z_float64| <= 1e-6 for EVERY ua (the bound the task noise needs: orr_task.h; 5.1e-7 in a host emulation of this code and 7.7e-7
// provable, profiles/init_noise.txt; measured by tests/test_gpu_init_noise.py).  1 - ua is exact and lies in [2^-24, 1], so r is finite and at most 5.77.  What float32 cannot do here:
// r reaches 5.77, where its own rounding is 2.4e-7 and that of the product another 2.4e-7, so a 1-ulp logarithm (v_log_f32, which also
// loses RELATIVE accuracy next to 1, i.e. for small ua), a 1-ulp square root and a float32 2 pi ub (3.7e-7 of angle at 5.77) each take
// the rest of the budget on their own.  So: the radius in float64 - ln(1 - ua) = e ln 2 + 2 atanh((m - 1) / (m + 1)) with the
// mantissa m in [sqrt 1/2, sqrt 2), seven terms of the series (|s| <= 0.172: 1e-12), reciprocal and square root from the hardware's
// float32 seeds (v_rcp_f32, v_rsq_f32) and one Newton step each - and the angle reduced EXACTLY: ub - k / 4 (k = the quarter turn) is
// a multiple of 2^-24 below 1/8, its product with a two-part 2 pi goes to joint_sincos as |a| <= pi / 4, the quarter turns are
// applied to the result.  What is left is joint_sincos' own error (6e-8) times r and the final rounding.  No libm, no branch; a few
// dozen f64 instructions, once per reset (sixteen lanes, a pair each) or once per target observation.
__device__ __forceinline__ void normal_pair(float ua, float ub, float* z0, float* z1) {
  const int wb = __float_as_int(1.0f - ua);                      // exact: 1 - ua = (2^24 - m) / 2^24, a normal float in [2^-24, 1]
  float mf = __int_as_float((wb & 0x007FFFFF) | 0x3F800000);     // mantissa in [1, 2)
  int e = (wb >> 23) - 127;
  const bool up = mf > 1.41421354f;
  mf = up ? 0.5f * mf : mf;
  e = up ? e + 1 : e;
  const double m = (double)mf, den = m + 1.0;
  double y = (double)__builtin_amdgcn_rcpf((float)den);          // 1 / (m + 1): 1e-7, one Newton step -> 1e-14
  y = y * (2.0 - den * y);
  const double s = (m - 1.0) * y, s2 = s * s;
  double p = 1.0 / 13.0;
  p = p * s2 + 1.0 / 11.0;
  p = p * s2 + 1.0 / 9.0;
  p = p * s2 + 1.0 / 7.0;
  p = p * s2 + 1.0 / 5.0;
  p = p * s2 + 1.0 / 3.0;
  p = p * s2 + 1.0;
  const double x = -2.0 * ((double)e * 0.69314718055994530942 + 2.0 * s * p);   // -2 ln(1 - ua) >= 0 (0 exactly for ua = 0: e = 0, s = 0)
  const double g = (double)__builtin_amdgcn_rsqf(fmaxf((float)x, 1e-30f));      // 1 / sqrt(x); ua = 0: a finite seed times x = 0
  double r = x * g;
  r = r + 0.5 * g * (x - r * r);                                                  // one Newton step
  const float k = rintf(4.0f * ub);                              // quarter turns, 0..4
  const float f = fmaf(-0.25f, k, ub);                           // exact, |f| <= 1/8
  const float a = fmaf(f, 6.2831854820251465f, f * -1.7484555e-07f);   // 2 pi f with a two-part 2 pi (as map_pi): half an ulp of a
  float sn, cs;
  joint_sincos(a, &sn, &cs);
  const int q = (int)k & 3;
  const float ss = (q & 1) ? cs : sn, cc = (q & 1) ? sn : cs;
  const float sq = (q & 2) ? -ss : ss, cq = ((q + 1) & 2) ? -cc : cc;
  *z0 = (float)(r * (double)cq);
  *z1 = (float)(r * (double)sq);
}

// Sine and cosine of the angle 2 pi u of one of the stream's 24-bit uniforms (u = m / 2^24 in [0, 1)), as normal_pair forms its angle:
// the quarter turn k = rint(4 u) comes off exactly (u - k / 4 is a multiple of 2^-24, |f| <= 1/8), the rest times a two-part 2 pi goes
// to joint_sincos as |a| <= pi / 4, the quarter turns are applied to the result.  Error: joint_sincos' own (< 1e-7) + half an ulp of a
// (orr_set_push: the heading of a kick)
__device__ __forceinline__ void unit_sincos(float u, float* sn, float* cs) {
  const float k = rintf(4.0f * u);                               // quarter turns, 0..4
  const float f = fmaf(-0.25f, k, u);                            // exact, |f| <= 1/8
  const float a = fmaf(f, 6.2831854820251465f, f * -1.7484555e-07f);   // 2 pi f with a two-part 2 pi (as map_pi)
  float s, c;
  joint_sincos(a, &s, &c);
  const int q = (int)k & 3;
  const float ss = (q & 1) ? c : s, cc = (q & 1) ? s : c;
  *sn = (q & 2) ? -ss : ss;
  *cs = ((q + 1) & 2) ? -cc : cc;
}

// ------------------------------------------------------------------------------------------------
// state helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int geti(const Shared& S, int off) { return __float_as_int(S.s[off]); }
__device__ __forceinline__ void seti(Shared& S, int off, int v) { S.s[off] = __int_as_float(v); }

}  // namespace orr
