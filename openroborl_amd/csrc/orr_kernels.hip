// orr_kernels.hip -- main translation unit of the env kernels (gfx950): the default kernels + the C-ABI of the vectorised quadruped
// imitation env.
//
// Hot path replaced: WrapperEnv.step / reset (wrapper_env.py:58-107) -> LocomotionGymEnv._step /
// reset (quadruped_gym_env.py:63-104,213-239) -> Minitaur (minitaur.py) + ImitationTask
// (imitation_task.py) + pybullet.stepSimulation.  One launch = one env step for all robots of
// this device: 33 physics sub-steps, observation, reward, termination, optional auto-reset.
// Specification of every stage: DESIGN.md section 4; CPU restatement: oracle/orr_oracle.c.
// The kernels and their launchers are templates in orr_env_kernels.h.  This unit instantiates the default ones (env step, debug
// physics, parity replay, reset) and launches all variants (which one: choose_variant, orr_variants.h); the two-wave, friction-anchor,
// clip-set, task-noise, reward-terms, contact-output, actuator, sensor-noise, randomiser and push instantiations are compiled in units of
// their own (orr_kernels_w2.hip, _anchor.hip, _multiclip.hip, _noise.hip, _terms.hip, _contacts.hip, _actuator.hip, _sensor.hip,
// _randomizer.hip, _push.hip; why: orr_env_kernels.h), and so is the privileged observation (_priv.hip).  Two small kernels that read the
// episode log live here as well: its pack for the rollout boundary (orr_episode_stats) and the clip curriculum (orr_clip_curriculum_update).
#define ORR_TU_MAIN 1
#include "orr_env_kernels.h"
#include "orr_variants.h"
#include <cstdarg>
// <0, ORR_WAVES_PER_EU>: one wave per SIMD in the shipped build; development builds (-DORR_WAVES_PER_EU=2 with the timers of this
// translation unit, tools/wave_pairing.py) get their instrumented two-wave kernel through the default path with ORR_STEP_WAVES_PER_EU=1
template orr::ResetLaunch orr::launch_reset<false>;
template orr::StepLaunch orr::launch_step<0, ORR_WAVES_PER_EU, false, false>;
template orr::StepLaunch orr::launch_step<1, ORR_WAVES_PER_EU, false, false>;
template orr::StepLaunch orr::launch_step<2, ORR_WAVES_PER_EU, false, false>;
#ifdef ORR_STAGE_DUMP
template orr::StageDumpLaunch orr::launch_stage_dump<false, 1>;     // development aid (orr_debug_stage_dump below)
template orr::StageDumpLaunch orr::launch_stage_dump<true, 1>;
#endif

// Rollout boundary (agents/ppo_imitation.py:405-423): pack this rank's episode log into the fixed-size float64 payload of the
// all-gather -- [n_listed, total_timesteps, n_dropped, n_episodes, sum_ret, sum_len, ret[K], len[K]] -- and clear the log, in
// ONE launch of one workgroup (the log holds at most a few ten thousand (return, length) pairs).
__global__ __launch_bounds__(1024) void orr_eplog_pack_kernel(long long* counters, const float* ep_log, int cap_log, double total_timesteps,
                                                              int K, double* out) {
  __shared__ double red_r[1024], red_l[1024];
  const int tid = threadIdx.x;
  const long long cnt_all = counters[ORR_CNT_EPISODES], dropped = counters[ORR_CNT_EPLOG_DROPPED];
  const long long cnt = cnt_all < (long long)cap_log ? cnt_all : (long long)cap_log;   // logged (the rest was counted as dropped)
  const float2* log2 = reinterpret_cast<const float2*>(ep_log);
  double sr = 0.0, sl = 0.0;
  for (long long i0 = tid; i0 < cnt; i0 += 4096) {   // four independent loads in flight per thread
    float2 e[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { const long long i = i0 + 1024 * u; e[u] = i < cnt ? log2[i] : make_float2(0.0f, 0.0f); }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const long long i = i0 + 1024 * u;
      sr += (double)e[u].x; sl += (double)e[u].y;
      if (i < cnt && i < K) { out[6 + i] = (double)e[u].x; out[6 + K + i] = (double)e[u].y; }
    }
  }
  for (long long i = cnt + tid; i < K; i += 1024) { out[6 + i] = 0.0; out[6 + K + i] = 0.0; }
  red_r[tid] = sr; red_l[tid] = sl;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (tid < w) { red_r[tid] += red_r[tid + w]; red_l[tid] += red_l[tid + w]; }
    __syncthreads();
  }
  if (tid == 0) {
    const long long listed = cnt < (long long)K ? cnt : (long long)K;
    out[0] = (double)listed; out[1] = total_timesteps; out[2] = (double)(dropped + (cnt - listed)); out[3] = (double)cnt;
    out[4] = red_r[0]; out[5] = red_l[0];
    counters[ORR_CNT_EPISODES] = 0; counters[ORR_CNT_EPLOG_DROPPED] = 0;   // every thread read them before the first barrier
  }
}

// The clip curriculum (orr_clip_curriculum_update, include/openroborl_hip.h): the episode log and the clip log as they stand -> per clip
// id the number n_c of logged episodes and the INTEGER sum S_c of their 16-bit scores, the running score ema_c, and the thresholds of
// every clip set of more than one clip (DevTables::clip_cum, what the multi-clip kernels draw by).  ONE launch of one workgroup; reads
// the logs and clears nothing.  The rows land in the log in the order the waves of a step finish, so everything that depends on more
// than one row is an integer sum: the result does not depend on the order of the rows.
// Phase 1, all threads: a row's (1, q) goes into the bin [clip][lane of the wave] of LDS with two non-returning integer atomics - the
// lanes of a wave hit 64 different words, so none of them serialises on an address.  Phase 2, 16 threads: one clip id each, its bins
// summed in a fixed order and the EMA in double.  Phase 3, one thread per robot type: the type's thresholds from the EMAs, in double.
__host__ __device__ __forceinline__ unsigned int uniform_threshold(int k, int n) {   // ceil(k 2^24 / n)
  return (unsigned int)((((unsigned long long)k << 24) + (unsigned long long)(n - 1)) / (unsigned long long)n); }
__global__ __launch_bounds__(1024) void orr_clip_curriculum_kernel(const long long* __restrict__ counters, const float* __restrict__ ep_log, int cap_log,
                                                                   const int* __restrict__ clip_log, DevTables* tab, double* stats) {
  __shared__ unsigned int bin_n[ORR_MAX_CLIPS][64];
  __shared__ unsigned long long bin_s[ORR_MAX_CLIPS][64];
  __shared__ double ema_s[ORR_MAX_CLIPS];
  __shared__ double f_s[ORR_MAX_ROBOT_TYPES][ORR_MAX_CLIPS];    // phase 3's per-entry weights (LDS, not a thread's array: no scratch)
  const int tid = threadIdx.x, slot = tid & 63;
  bin_n[tid >> 6][slot] = 0u; bin_s[tid >> 6][slot] = 0ull;      // 1024 threads = 16 x 64 bins
  const long long cnt_all = counters[ORR_CNT_EPISODES];
  const long long cnt = cnt_all < (long long)cap_log ? cnt_all : (long long)cap_log;   // logged rows (cap_log <= 0: none)
  const int metric = tab->cur.metric;
  __syncthreads();
  const float2* log2 = reinterpret_cast<const float2*>(ep_log);
  for (long long i0 = tid; i0 < cnt; i0 += 4096) {   // four independent rows in flight per thread
    float2 e[4];
    int cid[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const long long i = i0 + 1024 * u;
      e[u] = i < cnt ? log2[i] : make_float2(0.0f, 0.0f);
      cid[u] = i < cnt ? clip_log[i] : -1;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if ((unsigned int)cid[u] >= (unsigned int)ORR_MAX_CLIPS) continue;   // a clip id outside [0, 16): ignored (and the rows past cnt)
      const float x = metric == ORR_CLIP_METRIC_RETURN ? e[u].x : (metric == ORR_CLIP_METRIC_LENGTH ? e[u].y : __fdiv_rn(e[u].x, fmaxf(e[u].y, 1.0f)));
      const double r = fmin(fmax((double)x / (double)tab->cur.ref[cid[u]], 0.0), 1.0);   // NaN -> 0 (fmax returns its other argument)
      const unsigned int q = (unsigned int)floor(65536.0 * r + 0.5);
      atomicAdd(&bin_n[cid[u]][slot], 1u);
      atomicAdd(&bin_s[cid[u]][slot], (unsigned long long)q);
    }
  }
  __syncthreads();
  if (tid < ORR_MAX_CLIPS) {
    unsigned long long n = 0ull, s = 0ull;
    for (int j = 0; j < 64; j++) { n += bin_n[tid][j]; s += bin_s[tid][j]; }
    double ema = tab->cur.ema[tid];
    const double mean = n ? (double)s / (65536.0 * (double)n) : 0.0, alpha = (double)tab->cur.alpha;
    if (n) {
      ema = (1.0 - alpha) * ema + alpha * mean;
      tab->cur.ema[tid] = ema;
    }
    ema_s[tid] = ema;
    if (stats) { stats[4 * tid] = (double)n; stats[4 * tid + 1] = (double)s; stats[4 * tid + 2] = mean; stats[4 * tid + 3] = ema; }
  }
  __syncthreads();
  if (tid < ORR_MAX_ROBOT_TYPES) {
    int n = tab->clip_set_n[tid];
    n = n < ORR_MAX_CLIPS ? n : ORR_MAX_CLIPS;
    if (n > 1) {
      const double eps = (double)tab->cur.eps;
      double* const f = f_s[tid];
      double F = 0.0;
      for (int k = 0; k < n; k++) { f[k] = 1.0 - ema_s[tab->clip_set[tid][k] & (ORR_MAX_CLIPS - 1)]; F += f[k]; }
      unsigned int* cum = tab->clip_cum[tid];
      if (F < 1e-12) {
        for (int k = 0; k <= n; k++) cum[k] = uniform_threshold(k, n);
      } else {
        double P = 0.0;
        for (int k = 0; k < n; k++) { f[k] = (1.0 - eps) * f[k] / F + eps / (double)n; P += f[k]; }
        double Pk = 0.0;
        cum[0] = 0u;
        for (int k = 0; k < n; k++) { Pk += f[k]; cum[k + 1] = (unsigned int)ceil(16777216.0 * Pk / P); }
      }
    }
  }
}

// Policy-free stress input of SURVEY.md section 8d (i): action = (reference joint pose one control step ahead, taken from the first
// target frame of the observation, mapped joint -> motor space with the robot's own table) - INIT_MOTOR_ANGLES + noise, clipped to
// the action space (imitation_runners.py:140-143).  One thread per (robot, motor), ONE launch whatever the mix of robot types: a
// heterogeneous batch needs a per-robot permutation, which as tensor operations is a copy + a batched GEMM (three launches).
__global__ __launch_bounds__(256) void orr_stress_actions_kernel(const DevTables* __restrict__ tab, const float* __restrict__ state,
                                                                 const float* __restrict__ obs, const float* __restrict__ noise,
                                                                 float* __restrict__ actions, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n * 12) return;
  const int r = i / 12, m = i - 12 * r;
  const int type = __float_as_int(state[(size_t)r * ORR_STATE_STRIDE + ORR_OFF_ROBOT_TYPE]);
  const ModelCold& C = tab->model[type].cold;
  const float tar = obs[(size_t)r * ORR_OBS_DIM + 84 + 7 + C.joint_of_motor[m]];
  const float a = (tar - C.motor_offset[m]) * C.motor_dir[m] - C.init_motor_angles[m] + noise[i];
  actions[i] = fminf(fmaxf(a, -6.2831853f), 6.2831853f);
}

// ================================================================================================
// C-ABI (include/openroborl_hip.h)
// ================================================================================================
struct orr_handle {
  orr_config cfg;
  int simds;          // SIMDs of the device (4 per CU): a batch of more waves than that runs the two-waves-per-SIMD variant of the step kernel
  int force_wpe;      // ORR_STEP_WAVES_PER_EU (0 = automatic)
  uint32_t anchor_types;   // bit t = robot type t has orr_model::friction_anchor: launches run the ANCHOR variant of the step kernel
  uint32_t multiclip_types;   // bit t = robot type t has a clip set of more than one clip: orr_step / orr_reset run the multi-clip variants
  uint32_t switch_types;      // bit t = robot type t has a finite clip switch interval: the parity replays run the multi-clip variants
  bool noise_on;              // orr_set_task_noise: a probability or a heading deviation above 0: every entry point but the debug physics runs the noise variants
  bool terms_on;              // orr_bind_reward_terms: the steps run the terms variant (orr_kernels_terms.hip), the resets the noise variant
  bool contacts_on;           // orr_bind_contact_outputs: env step and debug physics run the contact variants (orr_kernels_contacts.hip), the resets the noise variant
  uint32_t limit_types;       // orr_set_torque_limits: bit t = robot type t has a finite torque limit on some motor
  bool act_on;                // orr_bind_actuator_outputs.  With either, env step and parity replay run the actuator variants (orr_kernels_actuator.hip), the resets the noise variant
  bool sensor_on;             // orr_set_sensor_noise: a motor-angle, rpy or rpy-rate deviation above 0: env step, parity replays and resets run the sensor variants (orr_kernels_sensor.hip)
  bool rand_on;               // orr_set_randomizer with a table (not NULL), or
  bool rand_bound;            // orr_bind_randomizer_params with a buffer: env step, parity replays and resets run the randomiser variants (orr_kernels_randomizer.hip)
  bool push_on;               // orr_set_push with prob > 0, or
  bool push_bound;            // orr_bind_push_outputs with a buffer: the env step runs the push variant (orr_kernels_push.hip); every other entry point launches what it launches without
  bool curriculum_on;         // orr_set_clip_curriculum gave settings: orr_clip_curriculum_update may launch (it selects no variant)
  bool shaping_on;            // orr_set_reward_shaping gave weights: orr_shaped_reward may launch (it selects no variant; orr_kernels_shaping.hip)
  DevTables* tab_dev;
  DevTables tab_host;
  float fb[3], fa[3];
  float* state;
  long long* counters;
  float* ep_log;
  int ep_log_cap;
  hipEvent_t ev0, ev1;
};

static thread_local char g_err[512] = "";
// records the message returned by orr_last_error(); shared with orr_policy.hip (same library)
__attribute__((visibility("hidden"))) int orr_fail(int code, const char* msg, hipError_t e) {
  if (e != hipSuccess) snprintf(g_err, sizeof(g_err), "%s: %s", msg, hipGetErrorString(e));
  else snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}
static int fail(int code, const char* msg, hipError_t e = hipSuccess) { return orr_fail(code, msg, e); }
#define HIPCHK(call, msg)                         \
  do {                                            \
    hipError_t e_ = (call);                       \
    if (e_ != hipSuccess) return fail(-2, msg, e_); \
  } while (0)

struct field_t { const char* name; int off, size, is_int; };
static const field_t g_fields[] = {
#define ORR_X_F(name, words, kind) {#name, ORR_OFF_##name, words, (#kind)[0] == 'I'},
    ORR_STATE_FIELDS(ORR_X_F)
#undef ORR_X_F
};

// The ABI carries times as float32; the reference computes with the DECIMAL constants of its sources in float64 (FrameDuration
// 0.01667, sim_time_step 0.001).  The shortest decimal (<= 7 significant digits) that rounds to the given float, else its exact value.
static double dec7(float x) {
  char b[40];
  snprintf(b, sizeof(b), "%.7g", (double)x);
  const double d = strtod(b, nullptr);
  return (float)d == x ? d : (double)x;
}

// The randomiser's parameters by name, in enum order, and the six ranges that reset_robot_state has built in
static const char* const g_rand_names[ORR_RAND_NUM_PARAMS] = {"base mass", "global motor strength", "inertia", "joint friction", "latency",
                                                              "lateral friction", "leg weaken", "mass", "motor strength", "single leg weaken"};
static orr_randomizer builtin_randomizer() {
  orr_randomizer r;
  memset(&r, 0, sizeof(r));
  const struct { int p; float lo, hi; } six[] = {{ORR_RAND_INERTIA, 0.5f, 1.5f}, {ORR_RAND_JOINT_FRICTION, 0.0f, 0.05f}, {ORR_RAND_LATENCY, 0.0f, 0.04f},
                                                 {ORR_RAND_LATERAL_FRICTION, 0.5f, 1.25f}, {ORR_RAND_MASS, 0.8f, 1.2f}, {ORR_RAND_MOTOR_STRENGTH, 0.8f, 1.2f}};
  for (const auto& e : six) { r.enabled[e.p] = 1; r.lo[e.p] = e.lo; r.hi[e.p] = e.hi; }
  return r;
}

// ---- what the setters of the C-ABI share.  Each of them goes: null handle, type range, validate, anchor conflict, device copy, host
// mirror, variant switch.  All of these return 0, or record the message and return the entry's code
__attribute__((format(printf, 1, 2))) static int refuse(const char* fmt, ...) {   // -1: a refused argument
  char m[sizeof(g_err)];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(m, sizeof(m), fmt, ap);
  va_end(ap);
  return fail(-1, m);
}
static int type_range(const char* entry, int32_t t) {
  return t < 0 || t >= ORR_MAX_ROBOT_TYPES ? refuse("%s: robot_type out of range", entry) : 0;
}
// the uniform thresholds of an n-entry clip set, in integer arithmetic; the entries past n are zero
static void uniform_thresholds(int n, unsigned int cum[ORR_MAX_CLIPS + 1]) {
  for (int k = 0; k <= ORR_MAX_CLIPS; k++) cum[k] = k <= n ? uniform_threshold(k, n) : 0u;
}
static void set_bit(uint32_t& mask, int t, bool on) { mask = on ? mask | 1u << t : mask & ~(1u << t); }
// the features that have no friction-anchor form of the kernels: refused while some robot type has orr_model::friction_anchor
static int anchor_conflict(const orr_handle* h, const char* entry, const char* what) {
  return h->anchor_types ? refuse("%s: friction anchors (orr_model::friction_anchor) and %s cannot be combined", entry, what) : 0;
}
struct named_value { const char* name; float v; };
template <size_t N> static int check_stds(const char* entry, const named_value (&table)[N]) {
  for (const auto& f : table)
    if (!(f.v >= 0.0f && f.v < INFINITY)) return refuse("%s: %s must be a finite standard deviation >= 0", entry, f.name);   // NaN fails the comparison
  return 0;
}
// `bytes` at src -> the member of the device table that mirrors host_field (a member of h->tab_host), then -> host_field.  The device
// copy first: a failed copy (-2, "<entry>: hipMemcpy: ...") leaves the host table, and the variant choice the caller makes next, as they were
static int upload(orr_handle* h, const char* entry, void* host_field, const void* src, size_t bytes) {
  void* dev_field = (char*)h->tab_dev + ((char*)host_field - (char*)&h->tab_host);
  const hipError_t e = hipMemcpy(dev_field, src, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    char m[96];
    snprintf(m, sizeof(m), "%s: hipMemcpy", entry);
    return fail(-2, m, e);
  }
  memcpy(host_field, src, bytes);
  return 0;
}
// The three output binds of a per-step buffer a (NULL = unbind: b and c are ignored), its per-episode companion b (required with a)
// and the per-episode log c (optional): three consecutive pointers of the tables from `first` on, and the handle's switch `flag`.
// needs_b / misaligned: the entry's own texts; misaligned = NULL where the buffers need no 16-byte alignment
static int bind_three(orr_handle* h, const char* entry, float* DevTables::*first, bool orr_handle::*flag, float* a, float* b, float* c,
                      const char* needs_b, const char* misaligned, const char* what) {
  if (!h) return refuse("%s: null handle", entry);
  const bool on = a != nullptr;
  if (on && !b) return refuse("%s: %s", entry, needs_b);
  if (on && misaligned && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) != 0) return refuse("%s: %s", entry, misaligned);
  if (on && anchor_conflict(h, entry, what)) return -1;
  float* p[3] = {a, on ? b : nullptr, on ? c : nullptr};
  if (const int r = upload(h, entry, &(h->tab_host.*first), p, sizeof(p))) return r;
  h->*flag = on;
  return 0;
}
#define ORR_THREE_POINTERS(a, b, c)                                                               \
  static_assert(offsetof(DevTables, b) == offsetof(DevTables, a) + sizeof(float*) &&              \
                offsetof(DevTables, c) == offsetof(DevTables, a) + 2 * sizeof(float*), "bind_three copies three consecutive pointers")

extern "C" {

#ifndef ORR_SOURCE_HASH
#define ORR_SOURCE_HASH "unknown"
#endif
const char* orr_last_error(void) { return g_err; }
int32_t orr_abi_version(void) { return ORR_ABI_VERSION; }
// "ORR_SRC_HASH=<hex>" is also what the host loader scans the FILE for (openroborl_amd/_lib.py: a stale-build check that must not dlopen)
static const char g_src_hash[] = "ORR_SRC_HASH=" ORR_SOURCE_HASH;
const char* orr_source_hash(void) { return g_src_hash + 13; }
int32_t orr_state_stride(void) { return ORR_STATE_STRIDE; }
int32_t orr_layout_count(void) { return (int32_t)(sizeof(g_fields) / sizeof(g_fields[0])); }
const char* orr_layout_name(int32_t i) { return g_fields[i].name; }
int32_t orr_layout_offset(int32_t i) { return g_fields[i].off; }
int32_t orr_layout_size(int32_t i) { return g_fields[i].size; }
int32_t orr_layout_is_int(int32_t i) { return g_fields[i].is_int; }
int32_t orr_sizeof_config(void) { return (int32_t)sizeof(orr_config); }
int32_t orr_sizeof_model(void) { return (int32_t)sizeof(orr_model); }
int32_t orr_sizeof_task_noise(void) { return (int32_t)sizeof(orr_task_noise); }
int32_t orr_sizeof_sensor_noise(void) { return (int32_t)sizeof(orr_sensor_noise); }
int32_t orr_sizeof_randomizer(void) { return (int32_t)sizeof(orr_randomizer); }
int32_t orr_sizeof_push(void) { return (int32_t)sizeof(orr_push); }

int32_t orr_create(const orr_config* cfg, orr_handle** out) {
  if (!cfg || !out) return fail(-1, "orr_create: null argument");
  if (cfg->abi_version != ORR_ABI_VERSION) return fail(-1, "orr_create: ABI version mismatch");
  if (cfg->num_robots < 1) return fail(-1, "orr_create: num_robots must be >= 1");
  if (cfg->action_repeat < 1 || cfg->solver_iters < 1) return fail(-1, "orr_create: action_repeat / solver_iters must be >= 1");
  // the quaternion update uses series for sin / cos of half the rotation of one sub-step (exact to float precision below 0.2 rad):
  // |w| <= sqrt(3) max_coord_velocity after the coordinate-velocity clamp
  if (!(cfg->max_coord_velocity > 0.0f) || !(cfg->sim_dt > 0.0f) || 0.5f * 1.7320508f * cfg->max_coord_velocity * cfg->sim_dt >= 0.2f)
    return fail(-1, "orr_create: max_coord_velocity * sim_dt too large (the base may turn at most 0.4 rad per sub-step)");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1) return fail(-3, "orr_create: no HIP device available (this library has no CPU fallback)", e);
  orr_handle* h = new orr_handle();
  memset(h, 0, sizeof(*h));
  h->cfg = *cfg;
  // ActionFilterButter.butter_filter (action_filter.py:196-217): scipy.signal.butter(2, [4 / (fs / 2)], 'low')
  {
    const double fs = 1.0 / ((double)cfg->sim_dt * cfg->action_repeat), wn = 4.0 / (0.5 * fs);
    const double K = tan(M_PI * wn / 2.0), K2 = K * K, den = 1.0 + sqrt(2.0) * K + K2;
    h->fb[0] = (float)(K2 / den); h->fb[1] = (float)(2.0 * K2 / den); h->fb[2] = (float)(K2 / den);
    h->fa[0] = 1.0f; h->fa[1] = (float)(2.0 * (K2 - 1.0) / den); h->fa[2] = (float)((1.0 - sqrt(2.0) * K + K2) / den);
  }
  {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    h->simds = 4 * cus;
    const char* f = getenv("ORR_STEP_WAVES_PER_EU");
    h->force_wpe = (f && (f[0] == '1' || f[0] == '2') && f[1] == 0) ? f[0] - '0' : 0;
  }
  // the initial table: zeros (the memset of the handle above) but for these three, and the device's copy of it
  for (int t = 0; t < ORR_MAX_ROBOT_TYPES; t++) {
    h->tab_host.clip_switch[t][0] = h->tab_host.clip_switch[t][1] = INFINITY;   // no switching
    for (int i = 0; i < 12; i++) h->tab_host.torque_limit[t][i] = INFINITY;     // no torque limit
  }
  h->tab_host.rnd = builtin_randomizer();   // what a bound params buffer applies until orr_set_randomizer gives a table
  const char* what = "orr_create: hipMalloc";
  e = hipMalloc((void**)&h->tab_dev, sizeof(DevTables));
  if (e == hipSuccess) {
    what = "orr_create: hipMemcpy";
    e = hipMemcpy(h->tab_dev, &h->tab_host, sizeof(DevTables), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) { hipFree(h->tab_dev); delete h; return fail(-2, what, e); }   // tab_dev is NULL where the allocation failed
  hipEventCreate(&h->ev0);
  hipEventCreate(&h->ev1);
  *out = h;
  return 0;
}

int32_t orr_set_seed(orr_handle* h, uint64_t seed) {
  if (!h) return fail(-1, "orr_set_seed: null handle");
  h->cfg.seed = seed;  // read by the next launch: the RNG is counter-based, keyed by (seed, robot index, episode index)
  return 0;
}

int32_t orr_destroy(orr_handle* h) {
  if (!h) return 0;
  hipFree(h->tab_dev);
  hipEventDestroy(h->ev0);
  hipEventDestroy(h->ev1);
  delete h;
  return 0;
}

int32_t orr_set_model(orr_handle* h, int32_t robot_type, const orr_model* m) {
  if (!h || !m) return fail(-1, "orr_set_model: null argument");
  if (type_range("orr_set_model", robot_type)) return -1;
  if (m->num_fall_proxies < 0 || m->num_fall_proxies > ORR_MAX_FALL_PROXIES) return fail(-1, "orr_set_model: bad num_fall_proxies");
  for (int i = 0; i < 12; i++) {
    if (m->joint_of_motor[i] < 0 || m->joint_of_motor[i] > 11) return fail(-1, "orr_set_model: joint_of_motor out of range");
    if (m->link_group[i] < 0 || m->link_group[i] > 1) return fail(-1, "orr_set_model: link_group must be 0 or 1");
  }
  for (int i = 0; i < m->num_fall_proxies; i++)
    if (m->fall_body[i] < 0 || m->fall_body[i] > 12) return fail(-1, "orr_set_model: fall_body out of range");
  // every joint must turn about a coordinate axis of the kinematic frame: hip about +-x, upper / lower leg about +-y
  // built in a local entry: a rejected model leaves the handle (host table, device table, anchor bit) exactly as it was
  DevModel d;
  memset(&d, 0, sizeof(d));
  float axsgn[12];
  for (int j = 0; j < 12; j++) {
    const int ax = (j % 3 == 0) ? 0 : 1;
    const float* a = m->joint_axis[j];
    for (int k = 0; k < 3; k++)
      if (k != ax && fabsf(a[k]) > 1e-6f) return fail(-1, "orr_set_model: joint axes must be +-x (hip) / +-y (upper, lower leg)");
    if (fabsf(fabsf(a[ax]) - 1.0f) > 1e-5f) return fail(-1, "orr_set_model: joint axis is not a unit coordinate axis");
    axsgn[j] = a[ax] > 0 ? 1.0f : -1.0f;
  }
  ModelHot& H = d.hot;
  ModelCold& Cd = d.cold;
  for (int i = 0; i < 3; i++) Cd.init_pos[i] = m->init_pos[i];
  for (int i = 0; i < 4; i++) H.init_quat[i] = m->init_quat[i];
  for (int i = 0; i < 12; i++) {
    const int j = m->joint_of_motor[i];
    Cd.init_motor_angles[i] = m->init_motor_angles[i];
    Cd.motor_dir[i] = m->motor_dir[i];
    Cd.motor_offset[i] = m->motor_offset[i];
    Cd.joint_of_motor[i] = j;
    Cd.kp[i] = m->kp[i];
    Cd.kd[i] = m->kd[i];
    if (fabsf(fabsf(m->motor_dir[i]) - 1.0f) > 1e-6f) return fail(-1, "orr_set_model: motor_dir must be +1 or -1");
    H.jdir[j] = m->motor_dir[i] * axsgn[j];
    H.joff[j] = m->motor_offset[i];
    Cd.tau_sign[j] = axsgn[j];
    Cd.tau_sign_motor[i] = axsgn[j];
    Cd.default_joints[i] = (m->init_motor_angles[i] + m->motor_offset[i]) * m->motor_dir[i];
  }
  for (int j = 0; j < 12; j++) {
    for (int k = 0; k < 3; k++) { Cd.link_com[j][k] = m->link_com[j][k]; H.joint_pos[j][k] = m->joint_pos[j][k]; }
    // limits are given for the kinematic angle; the internal angle is axis_sign times it
    H.joint_lo[j] = axsgn[j] > 0 ? m->joint_lo[j] : -m->joint_hi[j];
    H.joint_hi[j] = axsgn[j] > 0 ? m->joint_hi[j] : -m->joint_lo[j];
    if (!(H.joint_hi[j] - H.joint_lo[j] >= 2.0f * h->cfg.limit_activation))
      return fail(-1, "orr_set_model: joint range must be at least 2 * limit_activation");
  }
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 3; k++) { H.toe_pos[l][k] = m->toe_pos[l][k]; H.lower_com[l][k] = m->lower_com[l][k]; H.shank_pos[l][k] = m->shank_pos[l][k]; }
  if (!(m->shank_radius >= 0.0f)) return fail(-1, "orr_set_model: shank_radius must be >= 0");
  H.toe_radius = m->toe_radius;
  H.shank_radius = m->shank_radius;
  Cd.foot_friction = m->foot_friction;
  Cd.friction_anchor = m->friction_anchor != 0;
  if (m->friction_anchor && !(h->cfg.friction_erp >= 0.0f && h->cfg.friction_erp <= 1.0f)) return fail(-1, "orr_set_model: friction_anchor needs 0 <= orr_config::friction_erp <= 1");
  Cd.num_fall = m->num_fall_proxies;
  if (m->contact_stiffness > 0.0f) {
    if (!(m->contact_damping >= 0.0f)) return fail(-1, "orr_set_model: contact_damping must be >= 0");
    // btMultiBodyConstraintSolver::setupMultiBodyContactConstraint: cfm = 1 / (dt k + d), erp = dt k / (dt k + d); cfm *= 1 / dt
    const double dtk = (double)h->cfg.sim_dt * m->contact_stiffness, denom = dtk + m->contact_damping;
    H.contact_cfm = (float)(1.0 / denom / h->cfg.sim_dt);
    H.contact_erp_dt = (float)(dtk / denom / h->cfg.sim_dt);
  } else {
    H.contact_cfm = 0.0f;
    H.contact_erp_dt = h->cfg.contact_erp / h->cfg.sim_dt;
  }
  for (int i = 0; i < ORR_MAX_FALL_PROXIES; i++) {
    Cd.fall_body[i] = m->fall_body[i];
    Cd.fall_radius[i] = m->fall_radius[i];
    for (int k = 0; k < 3; k++) Cd.fall_pos[i][k] = m->fall_pos[i][k];
  }
  Cd.mass[0] = m->base_mass;
  Cd.group[0] = 0;
  for (int k = 0; k < 6; k++) { Cd.inertia[0][k] = m->base_inertia[k]; Cd.inertia_pa[0][k] = 0.0f; }
  for (int j = 0; j < 12; j++) {
    Cd.mass[j + 1] = m->link_mass[j];
    Cd.group[j + 1] = m->link_group[j];
    for (int k = 0; k < 6; k++) { Cd.inertia[j + 1][k] = m->link_inertia[j][k]; Cd.inertia_pa[j + 1][k] = m->link_inertia_pa[j][k]; }
  }
  if (const int r = upload(h, "orr_set_model", &h->tab_host.model[robot_type], &d, sizeof(d))) return r;
  set_bit(h->anchor_types, robot_type, m->friction_anchor != 0);
  return 0;
}

int32_t orr_set_motion(orr_handle* h, int32_t clip_id, const float* frames_dev, const float* frame_vels_dev, int32_t num_frames,
                       double frame_dt, int32_t clip_flags, const float cycle_delta[4]) {
  if (!h || !frames_dev || !frame_vels_dev || !cycle_delta) return fail(-1, "orr_set_motion: null argument");
  if (clip_id < 0 || clip_id >= ORR_MAX_CLIPS) return fail(-1, "orr_set_motion: clip_id out of range");
  if (num_frames < 2) return fail(-1, "orr_set_motion: need at least 2 frames");
  if (!(frame_dt > 0.0)) return fail(-1, "orr_set_motion: Frame duration must be positive.");
  DevClip c;
  c.frames = frames_dev; c.vels = frame_vels_dev; c.F = num_frames; c.flags = clip_flags;
  c.dt_d = frame_dt; c.dur_d = c.dt_d * (num_frames - 1); c.sim_dt_d = dec7(h->cfg.sim_dt);
  c.cdp[0] = cycle_delta[0]; c.cdp[1] = cycle_delta[1]; c.cdp[2] = cycle_delta[2]; c.cdh = cycle_delta[3];
  h->tab_host.clip[clip_id] = c;
  HIPCHK(hipMemcpy(&h->tab_dev->clip[clip_id], &c, sizeof(DevClip), hipMemcpyHostToDevice), "orr_set_motion: hipMemcpy");
  return 0;
}

int32_t orr_set_clip_set(orr_handle* h, int32_t robot_type, const int32_t* clip_ids_host, int32_t n) {
  if (!h || !clip_ids_host) return fail(-1, "orr_set_clip_set: null argument");
  if (type_range("orr_set_clip_set", robot_type)) return -1;
  if (n < 1 || n > ORR_MAX_CLIPS) return fail(-1, "orr_set_clip_set: a clip set holds 1 .. ORR_MAX_CLIPS clips");
  int ids[ORR_MAX_CLIPS] = {0};
  for (int i = 0; i < n; i++) {
    const int id = clip_ids_host[i];
    if (id < 0 || id >= ORR_MAX_CLIPS) return fail(-1, "orr_set_clip_set: clip id out of range");
    if (!h->tab_host.clip[id].frames) return fail(-1, "orr_set_clip_set: clip id was not loaded with orr_set_motion");
    ids[i] = id;
  }
  // a new set draws uniformly: thresholds ceil(k 2^24 / n), which pick (m n) >> 24 for every m
  unsigned int cum[ORR_MAX_CLIPS + 1];
  uniform_thresholds(n, cum);
  // the device copy first: a failed copy leaves the host table and the variant choice as they were
  HIPCHK(hipMemcpy(&h->tab_dev->clip_cum[robot_type][0], cum, sizeof(cum), hipMemcpyHostToDevice), "orr_set_clip_set: hipMemcpy");
  HIPCHK(hipMemcpy(&h->tab_dev->clip_set[robot_type][0], ids, sizeof(ids), hipMemcpyHostToDevice), "orr_set_clip_set: hipMemcpy");
  HIPCHK(hipMemcpy(&h->tab_dev->clip_set_n[robot_type], &n, sizeof(int), hipMemcpyHostToDevice), "orr_set_clip_set: hipMemcpy");
  memcpy(h->tab_host.clip_set[robot_type], ids, sizeof(ids));
  h->tab_host.clip_set_n[robot_type] = n;
  set_bit(h->multiclip_types, robot_type, n > 1);
  return 0;
}

// thresholds -> the device table only: the host's mirror of clip_cum is never read (the curriculum's kernel writes the device's copy)
static int put_thresholds(orr_handle* h, const char* entry, int robot_type, const unsigned int* cum) {
  const hipError_t e = hipMemcpy(&h->tab_dev->clip_cum[robot_type][0], cum, (ORR_MAX_CLIPS + 1) * sizeof(unsigned int), hipMemcpyHostToDevice);
  if (e == hipSuccess) return 0;
  char m[96];
  snprintf(m, sizeof(m), "%s: hipMemcpy", entry);
  return fail(-2, m, e);
}

int32_t orr_set_clip_weights(orr_handle* h, int32_t robot_type, const float* weights_host, int32_t n) {
  if (!h) return fail(-1, "orr_set_clip_weights: null handle");
  if (type_range("orr_set_clip_weights", robot_type)) return -1;
  const int set_n = h->tab_host.clip_set_n[robot_type];
  if (set_n < 1) return fail(-1, "orr_set_clip_weights: the robot type has no clip set (orr_set_clip_set)");
  if (n != set_n) return refuse("orr_set_clip_weights: %d weights for a clip set of %d entries", n, set_n);
  unsigned int cum[ORR_MAX_CLIPS + 1];
  uniform_thresholds(set_n, cum);
  if (weights_host) {
    double W = 0.0;
    for (int k = 0; k < n; k++) {
      if (!(weights_host[k] >= 0.0f && weights_host[k] < INFINITY)) return refuse("orr_set_clip_weights: weights_host[%d] must be a finite number >= 0", k);   // NaN fails the comparison
      W += (double)weights_host[k];
    }
    if (!(W > 0.0)) return fail(-1, "orr_set_clip_weights: all weights are zero");
    double Wk = 0.0;
    for (int k = 0; k < n; k++) { Wk += (double)weights_host[k]; cum[k + 1] = (unsigned int)ceil(16777216.0 * Wk / W); }
  }
  return put_thresholds(h, "orr_set_clip_weights", robot_type, cum);
}

int32_t orr_get_clip_thresholds(orr_handle* h, int32_t robot_type, uint32_t out_host[ORR_MAX_CLIPS + 1], int32_t* n) {
  if (!h || !out_host || !n) return fail(-1, "orr_get_clip_thresholds: null argument");
  if (type_range("orr_get_clip_thresholds", robot_type)) return -1;
  HIPCHK(hipDeviceSynchronize(), "orr_get_clip_thresholds: sync");     // the curriculum's kernel may still be writing them
  HIPCHK(hipMemcpy(out_host, &h->tab_dev->clip_cum[robot_type][0], (ORR_MAX_CLIPS + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost), "orr_get_clip_thresholds: hipMemcpy");
  *n = h->tab_host.clip_set_n[robot_type];
  return 0;
}

int32_t orr_sizeof_clip_curriculum(void) { return (int32_t)sizeof(orr_clip_curriculum); }

int32_t orr_set_clip_curriculum(orr_handle* h, const orr_clip_curriculum* cur_host) {
  if (!h || !cur_host) return fail(-1, "orr_set_clip_curriculum: null argument");
  const orr_clip_curriculum& c = *cur_host;
  if (!(c.alpha > 0.0f && c.alpha <= 1.0f)) return fail(-1, "orr_set_clip_curriculum: alpha must lie in (0, 1]");     // NaN fails the comparisons
  if (!(c.eps >= 0.0f && c.eps <= 1.0f)) return fail(-1, "orr_set_clip_curriculum: eps must lie in [0, 1]");
  if (c.metric != ORR_CLIP_METRIC_LENGTH && c.metric != ORR_CLIP_METRIC_RETURN && c.metric != ORR_CLIP_METRIC_STEP_REWARD)
    return fail(-1, "orr_set_clip_curriculum: unknown metric");
  for (int t = 0; t < ORR_MAX_ROBOT_TYPES; t++)
    for (int k = 0; k < h->tab_host.clip_set_n[t]; k++) {
      const int id = h->tab_host.clip_set[t][k];
      if (!(c.ref[id] > 0.0f && c.ref[id] < INFINITY)) return refuse("orr_set_clip_curriculum: ref[%d] must be finite and > 0 (the clip is in a clip set)", id);
    }
  DevTables::ClipCurriculum d;
  memset(&d, 0, sizeof(d));      // the EMAs start at zero
  d.alpha = c.alpha; d.eps = c.eps; d.metric = c.metric;
  memcpy(d.ref, c.ref, sizeof(d.ref));
  if (const int r = upload(h, "orr_set_clip_curriculum", &h->tab_host.cur, &d, sizeof(d))) return r;
  h->curriculum_on = true;
  return 0;
}

int32_t orr_clip_curriculum_update(orr_handle* h, double* stats_dev, void* stream) {
  if (!h) return fail(-1, "orr_clip_curriculum_update: null handle");
  if (!h->counters || !h->ep_log) return fail(-1, "orr_clip_curriculum_update: needs a bound episode log (orr_bind)");
  if (!h->tab_host.clip_log) return fail(-1, "orr_clip_curriculum_update: needs a bound clip log (orr_bind_clip_log)");
  if (!h->curriculum_on) return fail(-1, "orr_clip_curriculum_update: needs settings (orr_set_clip_curriculum)");
  hipLaunchKernelGGL(orr_clip_curriculum_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, h->counters, h->ep_log, h->ep_log_cap, h->tab_host.clip_log,
                     h->tab_dev, stats_dev);
  HIPCHK(hipGetLastError(), "orr_clip_curriculum_update: launch");
  return 0;
}

int32_t orr_bind_clip_log(orr_handle* h, int32_t* clip_log_dev) {
  if (!h) return fail(-1, "orr_bind_clip_log: null handle");
  int* p = clip_log_dev;
  return upload(h, "orr_bind_clip_log", &h->tab_host.clip_log, &p, sizeof(p));
}

int32_t orr_bind_reward_terms(orr_handle* h, float* terms_dev, float* term_sums_dev, float* term_log_dev) {
  ORR_THREE_POINTERS(terms, term_sums, term_log);
  return bind_three(h, "orr_bind_reward_terms", &DevTables::terms, &orr_handle::terms_on, terms_dev, term_sums_dev, term_log_dev,
                    "terms_dev needs term_sums_dev (the running sums of the current episode)", nullptr, "reward terms");
}

int32_t orr_bind_contact_outputs(orr_handle* h, float* contact_dev, float* contact_ep_dev, float* contact_log_dev) {
  ORR_THREE_POINTERS(contact_out, contact_ep, contact_log);
  return bind_three(h, "orr_bind_contact_outputs", &DevTables::contact_out, &orr_handle::contacts_on, contact_dev, contact_ep_dev, contact_log_dev,
                    "contact_dev needs contact_ep_dev (the totals of the current episode)",
                    "the contact buffers must be 16-byte aligned (rows of 16 and 8 floats)", "contact outputs");
}

int32_t orr_bind_actuator_outputs(orr_handle* h, float* act_dev, float* act_ep_dev, float* act_log_dev) {
  ORR_THREE_POINTERS(act_out, act_ep, act_log);
  return bind_three(h, "orr_bind_actuator_outputs", &DevTables::act_out, &orr_handle::act_on, act_dev, act_ep_dev, act_log_dev,
                    "act_dev needs act_ep_dev (the totals of the current episode)",
                    "the actuator buffers (act_dev, act_ep_dev, act_log_dev) must be 16-byte aligned (rows of 4 floats)", "actuator outputs");
}

int32_t orr_set_torque_limits(orr_handle* h, int32_t robot_type, const float* limits_host) {
  if (!h) return fail(-1, "orr_set_torque_limits: null handle");
  if (type_range("orr_set_torque_limits", robot_type)) return -1;
  float v[12];
  bool finite = false;
  for (int i = 0; i < 12; i++) {
    v[i] = limits_host ? limits_host[i] : INFINITY;
    if (!(v[i] >= 0.0f)) return refuse("orr_set_torque_limits: limits_host[%d] must be a torque >= 0 or +inf (no limit)", i);   // NaN fails the comparison
    finite = finite || v[i] < INFINITY;
  }
  if (finite && anchor_conflict(h, "orr_set_torque_limits", "torque limits")) return -1;
  if (const int r = upload(h, "orr_set_torque_limits", h->tab_host.torque_limit[robot_type], v, sizeof(v))) return r;
  set_bit(h->limit_types, robot_type, finite);
  return 0;
}

int32_t orr_set_clip_switch(orr_handle* h, int32_t robot_type, float tmin, float tmax) {
  if (!h) return fail(-1, "orr_set_clip_switch: null handle");
  if (type_range("orr_set_clip_switch", robot_type)) return -1;
  if (isnan(tmin) || isnan(tmax)) return fail(-1, "orr_set_clip_switch: NaN bound");
  if (tmin < 0.0f || tmax < 0.0f) return fail(-1, "orr_set_clip_switch: negative bound");
  if (tmin > tmax) return fail(-1, "orr_set_clip_switch: tmin > tmax");
  const bool off = isinf(tmin) && isinf(tmax);
  if (!off && (isinf(tmin) || isinf(tmax))) return fail(-1, "orr_set_clip_switch: both bounds finite, or both +inf (off)");
  if (!off && anchor_conflict(h, "orr_set_clip_switch", "clip switching")) return -1;
  const float v[2] = {tmin, tmax};
  if (const int r = upload(h, "orr_set_clip_switch", h->tab_host.clip_switch[robot_type], v, sizeof(v))) return r;
  set_bit(h->switch_types, robot_type, !off);
  return 0;
}

int32_t orr_set_task_noise(orr_handle* h, const orr_task_noise* noise_host) {
  if (!h) return fail(-1, "orr_set_task_noise: null handle");
  orr_task_noise n;
  memset(&n, 0, sizeof(n));
  if (noise_host) n = *noise_host;
  const named_value stds[] = {
      {"root_pos_std", n.root_pos_std}, {"root_rot_std", n.root_rot_std}, {"joint_pose_std", n.joint_pose_std}, {"root_vel_std", n.root_vel_std},
      {"root_ang_vel_std", n.root_ang_vel_std}, {"joint_vel_std", n.joint_vel_std}, {"tar_heading_std", n.tar_heading_std}};
  if (!(n.perturb_init_state_prob >= 0.0f && n.perturb_init_state_prob <= 1.0f))      // NaN fails the comparison
    return fail(-1, "orr_set_task_noise: perturb_init_state_prob must be a probability in [0, 1]");
  if (check_stds("orr_set_task_noise", stds)) return -1;
  const bool on = n.perturb_init_state_prob > 0.0f || n.tar_heading_std > 0.0f;
  if (on && anchor_conflict(h, "orr_set_task_noise", "task noise")) return -1;
  if (const int r = upload(h, "orr_set_task_noise", &h->tab_host.noise, &n, sizeof(n))) return r;
  h->noise_on = on;
  return 0;
}

int32_t orr_set_sensor_noise(orr_handle* h, const orr_sensor_noise* noise_host) {
  if (!h) return fail(-1, "orr_set_sensor_noise: null handle");
  orr_sensor_noise n;
  memset(&n, 0, sizeof(n));
  if (noise_host) n = *noise_host;
  const named_value stds[] = {
      {"motor_angle_std", n.motor_angle_std}, {"motor_velocity_std", n.motor_velocity_std}, {"motor_torque_std", n.motor_torque_std},
      {"base_rpy_std", n.base_rpy_std}, {"base_rpy_rate_std", n.base_rpy_rate_std}};
  if (check_stds("orr_set_sensor_noise", stds)) return -1;
  const bool on = n.motor_angle_std > 0.0f || n.base_rpy_std > 0.0f || n.base_rpy_rate_std > 0.0f;
  if (on && anchor_conflict(h, "orr_set_sensor_noise", "sensor noise")) return -1;
  if (const int r = upload(h, "orr_set_sensor_noise", &h->tab_host.sensor, &n, sizeof(n))) return r;
  h->sensor_on = on;
  return 0;
}

// DevTables::push_table follows rand_on / rand_bound: whether the push variant's auto-reset is the table-driven one
static int32_t sync_push_table(orr_handle* h, const char* entry) {
  const int t = h->rand_on || h->rand_bound ? 1 : 0;
  return t == h->tab_host.push_table ? 0 : upload(h, entry, &h->tab_host.push_table, &t, sizeof(t));
}

int32_t orr_set_randomizer(orr_handle* h, const orr_randomizer* host) {
  if (!h) return fail(-1, "orr_set_randomizer: null handle");
  orr_randomizer r = host ? *host : builtin_randomizer();
  // the ring reader (ctrl_obs / ring_prefetch, orr_robot_io.h) blends the entries n = int(latency / sim_dt) and n + 1 back from the
  // newest one, and clamps to the oldest where n + 1 >= the ring's length: exact while n + 1 <= ORR_RING_DEPTH - 1
  const float latency_max = (float)(ORR_RING_DEPTH - 2) * h->cfg.sim_dt;
  for (int p = 0; p < ORR_RAND_NUM_PARAMS; p++) {
    r.enabled[p] = r.enabled[p] != 0;
    if (!r.enabled[p]) { r.lo[p] = r.hi[p] = 0.0f; continue; }   // not read: kept as zeros
    const float lo = r.lo[p], hi = r.hi[p];
    const bool positive = p == ORR_RAND_BASE_MASS || p == ORR_RAND_MASS || p == ORR_RAND_INERTIA;
    const char* why = nullptr;
    if (!(fabsf(lo) < INFINITY && fabsf(hi) < INFINITY)) why = "bounds must be finite numbers";     // NaN fails the comparison
    else if (lo > hi) why = "lo > hi";
    else if (positive && !(lo > 0.0f)) why = "lo must be > 0 (a ratio of a mass or an inertia)";
    else if (lo < 0.0f) why = "lo must be >= 0";
    else if (p == ORR_RAND_LATENCY && hi > latency_max) why = "hi is beyond what the latency ring holds, (ORR_RING_DEPTH - 2) * sim_dt";
    if (why) return refuse("orr_set_randomizer: %s: %s", g_rand_names[p], why);
  }
  if (host && anchor_conflict(h, "orr_set_randomizer", "a randomiser table")) return -1;
  if (const int e = upload(h, "orr_set_randomizer", &h->tab_host.rnd, &r, sizeof(r))) return e;
  h->rand_on = host != nullptr;
  return sync_push_table(h, "orr_set_randomizer");
}

int32_t orr_bind_randomizer_params(orr_handle* h, float* params_dev, int32_t suspend) {
  if (!h) return fail(-1, "orr_bind_randomizer_params: null handle");
  if (((uintptr_t)params_dev & 15u) != 0) return fail(-1, "orr_bind_randomizer_params: params_dev must be 16-byte aligned (rows of ORR_RAND_ROW floats)");
  if (params_dev && anchor_conflict(h, "orr_bind_randomizer_params", "a randomiser params buffer")) return -1;
  struct { float* p; int s; } v = {params_dev, params_dev && suspend ? 1 : 0};
  static_assert(offsetof(DevTables, rand_suspend) == offsetof(DevTables, rand_params) + sizeof(float*), "copied as a pointer and the word behind it");
  if (const int r = upload(h, "orr_bind_randomizer_params", &h->tab_host.rand_params, &v, sizeof(float*) + sizeof(int))) return r;
  h->rand_bound = params_dev != nullptr;
  return sync_push_table(h, "orr_bind_randomizer_params");
}

int32_t orr_set_push(orr_handle* h, const orr_push* push_host) {
  if (!h) return fail(-1, "orr_set_push: null handle");
  orr_push p;
  memset(&p, 0, sizeof(p));
  if (push_host) p = *push_host;
  const float vmax = h->cfg.max_coord_velocity;   // the physics clamps every coordinate velocity there: a larger kick would not arrive
  const struct { const char* name; float v; bool speed; } fields[] = {
      {"prob", p.prob, false}, {"lin_lo", p.lin_lo, true}, {"lin_hi", p.lin_hi, true}, {"lin_z", p.lin_z, true}, {"ang", p.ang, true}};
  for (const auto& f : fields) {      // its own wordings, not check_stds': a probability and four speeds
    const char* why = nullptr;
    if (!(fabsf(f.v) < INFINITY)) why = "must be a finite number";      // NaN fails the comparison
    else if (f.v < 0.0f) why = "must be >= 0";
    else if (!f.speed && f.v > 1.0f) why = "must be a probability in [0, 1]";
    else if (f.speed && f.v > vmax) why = "is above orr_config::max_coord_velocity";
    if (why) return refuse("orr_set_push: %s %s", f.name, why);
  }
  if (p.lin_lo > p.lin_hi) return fail(-1, "orr_set_push: lin_lo > lin_hi");
  if (p.grace_steps < 0) return fail(-1, "orr_set_push: grace_steps must be >= 0");
  const bool on = p.prob > 0.0f;
  if (on && anchor_conflict(h, "orr_set_push", "pushes")) return -1;
  if (const int r = upload(h, "orr_set_push", &h->tab_host.push, &p, sizeof(p))) return r;
  h->push_on = on;
  return 0;
}

int32_t orr_bind_push_outputs(orr_handle* h, float* push_dev) {
  if (!h) return fail(-1, "orr_bind_push_outputs: null handle");
  if (((uintptr_t)push_dev & 15u) != 0) return fail(-1, "orr_bind_push_outputs: push_dev must be 16-byte aligned (rows of ORR_PUSH_ROW floats)");
  if (push_dev && anchor_conflict(h, "orr_bind_push_outputs", "push outputs")) return -1;
  if (const int r = upload(h, "orr_bind_push_outputs", &h->tab_host.push_out, &push_dev, sizeof(push_dev))) return r;
  h->push_bound = push_dev != nullptr;
  return 0;
}

int32_t orr_bind(orr_handle* h, void* state_dev, int64_t* counters_dev, float* ep_log_dev, int32_t ep_log_capacity) {
  if (!h || !state_dev || !counters_dev) return fail(-1, "orr_bind: null argument (state and counters are required)");
  if (((uintptr_t)state_dev & 15u) != 0) return fail(-1, "orr_bind: the state buffer must be 16-byte aligned (records move in 16-byte pieces)");
  h->state = (float*)state_dev;
  h->counters = (long long*)counters_dev;
  h->ep_log = ep_log_dev;
  h->ep_log_cap = ep_log_dev ? ep_log_capacity : 0;
  return 0;
}

#ifdef ORR_WAVE_TIMELINE
static long long* g_wave_times_dev = nullptr;
static int g_wave_times_cap = 0;
#endif
static KParams make_params(const orr_handle* h) {
  KParams P;
  P.cfg = h->cfg;
  for (int i = 0; i < 3; i++) { P.fb[i] = h->fb[i]; P.fa[i] = h->fa[i]; }
  P.tab = h->tab_dev;
  P.state = h->state;
  P.counters = h->counters;
  P.ep_log = h->ep_log;
  P.ep_log_cap = h->ep_log_cap;
  P.simds = h->simds;
  P.anchor_on = h->anchor_types != 0;
#ifdef ORR_WAVE_TIMELINE
  P.wave_times = g_wave_times_dev;
  P.wave_times_cap = g_wave_times_cap;
#endif
  return P;
}

static int waves_of(const orr_handle* h) { return (h->cfg.num_robots + kRPW - 1) / kRPW; }

// ---- which instantiation of the kernels a launch runs.  The rule is choose_variant (orr_variants.h); here: what it reads, and what each
// entry point launches for each answer ----
static Features features_of(const orr_handle* h, Entry e) {   // the one place that reads the handle's switches for the choice
  const bool replay = e == kEntryReplayStep || e == kEntryReplayReset;
  Features f;
  f.anchors = h->anchor_types != 0;
  f.clips = (replay ? h->switch_types : h->multiclip_types) != 0;
  f.noise = h->noise_on;
  f.terms = h->terms_on;
  f.contacts = h->contacts_on;
  f.actuator = h->act_on || h->limit_types;
  f.sensor = h->sensor_on;
  f.randomizer = h->rand_on || h->rand_bound;
  f.push = h->push_on || h->push_bound;
  f.two_wave = h->force_wpe ? h->force_wpe == 2 : waves_of(h) > h->simds;
  return f;
}
static Variant choose(const orr_handle* h, Entry e) {   // kRefused: the message is recorded, the caller returns -1
  const Choice c = choose_variant(features_of(h, e), e);
  if (c.variant == kRefused) {
    char m[256];
    format_anchor_conflict(m, sizeof(m), e, c.conflict);
    fail(-1, m);
  }
  return c.variant;
}

// The feature masks of the step kernels' MODE, each a superset of the one before it (the unit that instantiates each: the
// `extern template` lines of orr_env_kernels.h); the parity replays' (| 2) have no contact sums
constexpr int kStepTerms = kModeTerms, kStepContacts = kModeContacts, kStepContactsTerms = kModeContacts | kModeTerms,
              kStepActuator = kModeActuator | kStepContactsTerms, kStepSensor = kModeSensor | kStepActuator,
              kStepRandomizer = kModeRandomizer | kStepSensor, kStepPush = kModePush | kStepRandomizer;
constexpr int kReplayTerms = kModeTerms | 2, kReplayActuator = kModeActuator | kReplayTerms, kReplaySensor = kModeSensor | kReplayActuator,
              kReplayRandomizer = kModeRandomizer | kReplaySensor;

// One line per variant and entry point; a variant without a line fails to compile.  nullptr = choose_variant never gives it there.
#pragma clang diagnostic error "-Wswitch"
static StepLaunch* step_launcher(Variant v) {   // orr_step: the feature variants run one wave per SIMD at any batch size
  switch (v) {
    case kPush: return launch_step<kStepPush, 1, false, true, true>;
    case kRandomizer: return launch_step<kStepRandomizer, 1, false, true, true>;
    case kSensor: return launch_step<kStepSensor, 1, false, true, true>;
    case kActuator: return launch_step<kStepActuator, 1, false, true, true>;
    case kContactsTerms: return launch_step<kStepContactsTerms, 1, false, true, true>;
    case kContacts: return launch_step<kStepContacts, 1, false, true, true>;
    case kTerms: return launch_step<kStepTerms, 1, false, true, true>;
    case kNoise: return launch_step<0, 1, false, true, true>;
    case kClips: return launch_step<0, 1, false, true>;
    case kAnchor: return launch_step<0, 1, true, false>;
    case kTwoWave: return launch_step<0, 2, false, false>;
    case kDefault: return launch_step<0, ORR_WAVES_PER_EU, false, false>;
    case kRefused: case kNumVariants: break;
  }
  return nullptr;
}
static StepLaunch* replay_step_launcher(Variant v) {   // orr_debug_replay_step: no reset inside, no two-wave or anchor form
  switch (v) {
    case kRandomizer: return launch_step<kReplayRandomizer, 1, false, true, true>;   // (no reset inside: the sensor replay's computation)
    case kSensor: return launch_step<kReplaySensor, 1, false, true, true>;           // the noisy readings' draws come from the Philox stream
    case kActuator: return launch_step<kReplayActuator, 1, false, true, true>;
    case kTerms: return launch_step<kReplayTerms, 1, false, true, true>;
    case kNoise: return launch_step<2, 1, false, true, true>;   // the draws from 28 on, the heading noise included, come from the Philox stream
    case kClips: return launch_step<2, 1, false, true>;         // likewise
    case kAnchor: case kTwoWave: case kDefault: return launch_step<2, ORR_WAVES_PER_EU, false, false>;
    case kPush: case kContacts: case kContactsTerms: case kRefused: case kNumVariants: break;
  }
  return nullptr;
}
static StepLaunch* physics_launcher(Variant v) {   // orr_debug_physics: choose_variant gives it these three only
  switch (v) {
    case kContacts: return launch_step<kModeContacts | 1, 1, false, false>;   // also sums the nsub sub-steps' contact impulses
    case kAnchor: return launch_step<1, 1, true, false>;
    case kDefault: return launch_step<1, ORR_WAVES_PER_EU, false, false>;
    case kTwoWave: case kClips: case kNoise: case kTerms: case kContactsTerms: case kActuator: case kSensor: case kRandomizer: case kPush:
    case kRefused: case kNumVariants: break;
  }
  return nullptr;
}
static ResetLaunch* reset_launcher(Variant v) {   // orr_reset and, with the draws 0..27 given, orr_debug_replay_reset (where kContacts cannot occur)
  switch (v) {
    case kRandomizer: return launch_randomizer_reset<true>;   // the sensor reset with the table-driven randomiser
    case kSensor: return launch_sensor_reset<true>;           // three noisy readings per history, a noisy heading of the target observation
    case kNoise: case kTerms: case kContacts: case kActuator: return launch_reset<true, true>;   // perturbed initial states / noisy target heading, and the clip draw
    case kClips: return launch_reset<true>;                   // every reset draws the episode's clip
    case kAnchor: case kTwoWave: case kDefault: return launch_reset<false>;
    case kPush: case kContactsTerms: case kRefused: case kNumVariants: break;
  }
  return nullptr;
}

static int launch_failed(Entry e, Variant v, hipError_t err) {   // "<entry>: launch (<variant>)"
  static const char* const labels[] = {"", " (two waves per SIMD)", " (friction anchors)", " (clip sets)", " (task noise)", " (reward terms)", " (contact outputs)",
                                       " (contact outputs + reward terms)", " (actuator)", " (sensor noise)", " (randomiser)", " (push)"};
  static_assert(sizeof(labels) / sizeof(labels[0]) == kNumVariants, "one label per variant");
  char m[128];
  snprintf(m, sizeof(m), "%s: launch%s", kEntryNames[e], labels[v]);
  return fail(-2, m, err);
}
static int launch(const orr_handle* h, Entry e, Variant v, StepLaunch* fn, void* stream, const float* in, float* obs, float* reward, uint8_t* done, int nsub,
                  const ReplayArgs& rp) {
  const hipError_t err = fn ? fn(make_params(h), waves_of(h), (hipStream_t)stream, in, obs, reward, done, nsub, rp) : hipErrorInvalidDeviceFunction;
  return err == hipSuccess ? 0 : launch_failed(e, v, err);
}
static int launch(const orr_handle* h, Entry e, Variant v, ResetLaunch* fn, void* stream, const uint8_t* mask, float* obs, const float* uniforms) {
  const hipError_t err = fn ? fn(make_params(h), waves_of(h), (hipStream_t)stream, mask, obs, uniforms) : hipErrorInvalidDeviceFunction;
  return err == hipSuccess ? 0 : launch_failed(e, v, err);
}

int32_t orr_reset(orr_handle* h, const uint8_t* mask_dev, float* obs_dev, void* stream) {
  if (!h || !h->state) return fail(-1, "orr_reset: handle not bound");
  const Variant v = choose(h, kEntryReset);
  return v == kRefused ? -1 : launch(h, kEntryReset, v, reset_launcher(v), stream, mask_dev, obs_dev, nullptr);
}

int32_t orr_step(orr_handle* h, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream) {
  if (!h || !h->state) return fail(-1, "orr_step: handle not bound");
  if (!actions_dev || !obs_dev || !reward_dev || !done_dev) return fail(-1, "orr_step: null buffer");
  if (((uintptr_t)obs_dev & 15u) != 0) return fail(-1, "orr_step: the observation buffer must be 16-byte aligned (it is written in 16-byte pieces)");
  const Variant v = choose(h, kEntryStep);
  return v == kRefused ? -1 : launch(h, kEntryStep, v, step_launcher(v), stream, actions_dev, obs_dev, reward_dev, done_dev, 0, ReplayArgs{});
}

// the privileged observation: its kernel lives in orr_kernels_priv.hip (no variants: it reads the record and whatever outputs are bound)
int32_t orr_privileged_obs(orr_handle* h, const uint8_t* done_dev, float* priv_dev, void* stream) {
  if (!h) return fail(-1, "orr_privileged_obs: null handle");
  if (!priv_dev) return fail(-1, "orr_privileged_obs: null buffer");
  if (((uintptr_t)priv_dev & 15u) != 0) return fail(-1, "orr_privileged_obs: priv_dev must be 16-byte aligned (rows of ORR_PRIV_DIM floats, written in 16-byte pieces)");
  if (!h->state) return fail(-1, "orr_privileged_obs: handle not bound");
  const float lat_div = (float)(ORR_RING_DEPTH - 2) * h->cfg.sim_dt, step_dt = (float)h->cfg.action_repeat * h->cfg.sim_dt;
  HIPCHK(launch_privileged_obs(h->tab_dev, h->state, h->cfg.num_robots, done_dev, priv_dev, lat_div, step_dt, (hipStream_t)stream), "orr_privileged_obs: launch");
  return 0;
}

// reward shaping: its kernels live in orr_kernels_shaping.hip (no variants: a post-step kernel that reads the record, the bound actuator /
// contact outputs and the weights in the device table)
int32_t orr_sizeof_reward_shaping(void) { return (int32_t)sizeof(orr_reward_shaping); }

int32_t orr_set_reward_shaping(orr_handle* h, const orr_reward_shaping* host, void* stream) {
  if (!h) return fail(-1, "orr_set_reward_shaping: null handle");
  if (!h->state) return fail(-1, "orr_set_reward_shaping: handle not bound");
  orr_reward_shaping s;
  memset(&s, 0, sizeof(s));
  if (host) {
    s = *host;
    for (int k = 0; k < ORR_SHAPING_TERMS; k++)
      if (!(s.w[k] >= 0.0f && s.w[k] < INFINITY)) return refuse("orr_set_reward_shaping: w[%d] must be a finite number >= 0", k);   // NaN fails the comparison
    if (!(s.floor < INFINITY)) return fail(-1, "orr_set_reward_shaping: floor must be a number below +inf (-inf = none)");
  }
  // in stream order, without a synchronisation: a kernel that takes the seven words by value writes the device's copy
  HIPCHK(launch_set_shaping(h->tab_dev, s, (hipStream_t)stream), "orr_set_reward_shaping: launch");
  h->tab_host.shaping = s;
  h->shaping_on = host != nullptr;
  return 0;
}

int32_t orr_bind_reward_shaping(orr_handle* h, float* shape_dev, float* shape_ep_dev, float* shape_tot_dev, float* prev_dev) {
  static_assert(offsetof(DevTables, shape_ep) == offsetof(DevTables, shape_out) + sizeof(float*) &&
                offsetof(DevTables, shape_tot) == offsetof(DevTables, shape_out) + 2 * sizeof(float*) &&
                offsetof(DevTables, shape_prev) == offsetof(DevTables, shape_out) + 3 * sizeof(float*), "copied as four consecutive pointers");
  if (!h) return fail(-1, "orr_bind_reward_shaping: null handle");
  if (!h->state) return fail(-1, "orr_bind_reward_shaping: handle not bound");
  const bool on = shape_dev != nullptr;
  if (on && (!shape_ep_dev || !shape_tot_dev || !prev_dev))
    return fail(-1, "orr_bind_reward_shaping: shape_dev needs shape_ep_dev, shape_tot_dev and prev_dev");
  if (on && (((uintptr_t)shape_dev | (uintptr_t)shape_ep_dev | (uintptr_t)shape_tot_dev | (uintptr_t)prev_dev) & 15u) != 0)
    return fail(-1, "orr_bind_reward_shaping: the buffers must be 16-byte aligned (rows of 8 and 24 floats, read and written in 16-byte pieces)");
  float* p[4] = {shape_dev, on ? shape_ep_dev : nullptr, on ? shape_tot_dev : nullptr, on ? prev_dev : nullptr};
  return upload(h, "orr_bind_reward_shaping", &h->tab_host.shape_out, p, sizeof(p));
}

int32_t orr_shaped_reward(orr_handle* h, const float* actions_dev, const float* reward_in_dev, const uint8_t* done_dev, float* reward_out_dev,
                          void* stream) {
  if (!h) return fail(-1, "orr_shaped_reward: null handle");
  if (!actions_dev || !reward_in_dev || !done_dev || !reward_out_dev) return fail(-1, "orr_shaped_reward: null buffer");
  if (!h->state) return fail(-1, "orr_shaped_reward: handle not bound");
  if (!h->shaping_on) return fail(-1, "orr_shaped_reward: reward shaping is not set (orr_set_reward_shaping)");
  if (!h->tab_host.shape_out) return fail(-1, "orr_shaped_reward: the shaping buffers are not bound (orr_bind_reward_shaping)");
  if (((uintptr_t)actions_dev & 15u) != 0) return fail(-1, "orr_shaped_reward: actions_dev must be 16-byte aligned (rows of 12 floats, read in 16-byte pieces)");
  if ((((uintptr_t)reward_in_dev | (uintptr_t)reward_out_dev) & 3u) != 0) return fail(-1, "orr_shaped_reward: reward_in_dev and reward_out_dev must be 4-byte aligned");
  const orr_reward_shaping& s = h->tab_host.shaping;
  if ((s.w[ORR_SHAPING_TORQUE] != 0.0f || s.w[ORR_SHAPING_WORK] != 0.0f) && !h->tab_host.act_out)
    return fail(-1, "orr_shaped_reward: a torque or work weight needs bound actuator outputs (orr_bind_actuator_outputs)");
  if (s.w[ORR_SHAPING_IMPACT] != 0.0f && !h->tab_host.contact_out)
    return fail(-1, "orr_shaped_reward: an impact weight needs bound contact outputs (orr_bind_contact_outputs)");
  const float inv_nsub = 1.0f / (float)h->cfg.action_repeat, inv_dt = 1.0f / h->cfg.sim_dt;
  HIPCHK(launch_shaped_reward(h->tab_dev, h->state, h->cfg.num_robots, actions_dev, reward_in_dev, done_dev, reward_out_dev, inv_nsub, inv_dt,
                              (hipStream_t)stream), "orr_shaped_reward: launch");
  return 0;
}

// parity / debug entry point (not part of the drop-in surface): nsub physics sub-steps with fixed motor torques
int32_t orr_debug_physics(orr_handle* h, const float* torques_dev, uint8_t* fall_dev, int32_t nsub, void* stream) {
  if (!h || !h->state || !torques_dev) return fail(-1, "orr_debug_physics: bad argument");
  const Variant v = choose(h, kEntryDebugPhysics);
  return v == kRefused ? -1 : launch(h, kEntryDebugPhysics, v, physics_launcher(v), stream, torques_dev, nullptr, nullptr, fall_dev, nsub, ReplayArgs{});
}

int32_t orr_episode_stats(orr_handle* h, double total_timesteps, int32_t capacity, double* out_dev, void* stream) {
  if (!h || !h->counters || !h->ep_log || !out_dev) return fail(-1, "orr_episode_stats: needs a bound episode log and an output buffer");
  if (capacity < 1) return fail(-1, "orr_episode_stats: capacity must be >= 1");
  hipLaunchKernelGGL(orr_eplog_pack_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, h->counters, h->ep_log, h->ep_log_cap, total_timesteps,
                     (int)capacity, out_dev);
  HIPCHK(hipGetLastError(), "orr_episode_stats: launch");
  return 0;
}

// measurement input (not part of the drop-in surface): the policy-free stress actions of SURVEY.md section 8d (i), see the kernel
int32_t orr_stress_actions(orr_handle* h, const float* obs_dev, const float* noise_dev, float* actions_dev, void* stream) {
  if (!h || !h->state) return fail(-1, "orr_stress_actions: handle not bound");
  if (!obs_dev || !noise_dev || !actions_dev) return fail(-1, "orr_stress_actions: null buffer");
  const int n = h->cfg.num_robots;
  hipLaunchKernelGGL(orr_stress_actions_kernel, dim3((n * 12 + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->tab_dev, h->state, obs_dev,
                     noise_dev, actions_dev, n);
  HIPCHK(hipGetLastError(), "orr_stress_actions: launch");
  return 0;
}

// parity / debug entry points (not part of the drop-in surface): the env step / reset with the physics engine, the link
// positions, the contact flag and the random draws REPLAYED from buffers (see ReplayArgs in orr_device.h)
int32_t orr_debug_replay_step(orr_handle* h, const float* actions_dev, const float* traj_dev, const float* eff_dev, const uint8_t* fall_dev,
                              float* obs_dev, float* reward_dev, uint8_t* done_dev, float* tau_out_dev, void* stream) {
  if (!h || !h->state) return fail(-1, "orr_debug_replay_step: handle not bound");
  if (!actions_dev || !traj_dev || !eff_dev || !fall_dev || !obs_dev || !reward_dev || !done_dev || !tau_out_dev)
    return fail(-1, "orr_debug_replay_step: null buffer");
  if (h->cfg.flags & ORR_FLAG_AUTO_RESET) return fail(-1, "orr_debug_replay_step: needs a handle without ORR_FLAG_AUTO_RESET");
  const ReplayArgs rp{traj_dev, eff_dev, fall_dev, tau_out_dev, nullptr};
  const Variant v = choose(h, kEntryReplayStep);
  return v == kRefused ? -1 : launch(h, kEntryReplayStep, v, replay_step_launcher(v), stream, actions_dev, obs_dev, reward_dev, done_dev, 0, rp);
}
int32_t orr_debug_replay_reset(orr_handle* h, const float* uniforms_dev, float* obs_dev, void* stream) {
  if (!h || !h->state || !uniforms_dev) return fail(-1, "orr_debug_replay_reset: bad argument");
  const Variant v = choose(h, kEntryReplayReset);
  return v == kRefused ? -1 : launch(h, kEntryReplayReset, v, reset_launcher(v), stream, nullptr, obs_dev, uniforms_dev);
}

int32_t orr_time_steps(orr_handle* h, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream,
                       int32_t num_steps, float* total_ms_out) {
  if (!h || !h->state || !total_ms_out) return fail(-1, "orr_time_steps: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipEventRecord(h->ev0, st), "orr_time_steps: event");
  for (int i = 0; i < num_steps; i++) {
    int rc = orr_step(h, actions_dev, obs_dev, reward_dev, done_dev, stream);
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(h->ev1, st), "orr_time_steps: event");
  HIPCHK(hipEventSynchronize(h->ev1), "orr_time_steps: sync");
  HIPCHK(hipEventElapsedTime(total_ms_out, h->ev0, h->ev1), "orr_time_steps: elapsed");
  return 0;
}

#ifdef ORR_STAGE_DUMP
// development aid (-DORR_STAGE_DUMP; tests/test_gpu_substep_stages.py): what the first half of ONE physics sub-step hands from stage to
// stage (orr_stage_dump_kernel, orr_env_kernels.h), for the bound records as they are and the given motor torques [N][12]; the records
// are not changed.  out_dev takes orr_debug_stage_words() float32 words per robot.  The unit is the one whose step kernel the handle
// runs (batch size, ORR_STEP_WAVES_PER_EU), the friction-anchor form that of a handle with an anchor model.
int32_t orr_debug_stage_words(void) { return kStageWords; }
int32_t orr_debug_stage_dump(orr_handle* h, const float* torques_dev, float* out_dev, int64_t out_words, void* stream) {
  if (!h || !h->state) return fail(-1, "orr_debug_stage_dump: handle not bound");
  if (!torques_dev || !out_dev) return fail(-1, "orr_debug_stage_dump: null buffer");
  if (out_words < (int64_t)h->cfg.num_robots * kStageWords) return fail(-1, "orr_debug_stage_dump: out_words is less than num_robots * orr_debug_stage_words()");
  const bool two = h->force_wpe ? h->force_wpe == 2 : waves_of(h) > h->simds, anchor = h->anchor_types != 0;
  StageDumpLaunch* const launch = two ? (anchor ? launch_stage_dump<true, 2> : launch_stage_dump<false, 2>)
                                      : (anchor ? launch_stage_dump<true, 1> : launch_stage_dump<false, 1>);
  HIPCHK(launch(make_params(h), waves_of(h), (hipStream_t)stream, torques_dev, out_dev, (long long)out_words), "orr_debug_stage_dump: launch");
  return 0;
}
#endif
#if defined(ORR_COUNT_DUAL_CONTACT)
// development aid: read (and optionally clear) the toe / shank contact counters of the -DORR_COUNT_DUAL_CONTACT build
int orr_debug_dual_contact(unsigned long long* out8, int reset) {
  HIPCHK(hipDeviceSynchronize(), "orr_debug_dual_contact: sync");
  HIPCHK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_dual_contact), 8 * sizeof(unsigned long long)), "orr_debug_dual_contact: read");
  if (reset) {
    unsigned long long z[8] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_dual_contact), z, sizeof(z)), "orr_debug_dual_contact: clear");
  }
  return 0;
}
#endif
#ifdef ORR_WAVE_TIMELINE
// development aid (-DORR_WAVE_TIMELINE, which -DORR_PHASE_TIMERS implies): per-wave timeline of the last step launch of any variant (4 words per wave: realtime start / end in 100 MHz ticks,
// shader cycles, bits 0..7 mask of the robots that finished an episode | bits 8..39 HW_ID (wave slot, SIMD, CU, SE) | bits 40..43 XCC id).
// The first call (waves > 0, out may be null) allocates the device buffer; launches after it are recorded.
int orr_debug_wave_times(long long* out, int waves) {
  HIPCHK(hipDeviceSynchronize(), "orr_debug_wave_times: sync");
  if (waves > g_wave_times_cap) {
    g_wave_times_cap = 0;      // nothing is recorded until the new buffer stands
    if (g_wave_times_dev) HIPCHK(hipFree(g_wave_times_dev), "orr_debug_wave_times: free");
    g_wave_times_dev = nullptr;
    HIPCHK(hipMalloc((void**)&g_wave_times_dev, (size_t)waves * 4 * sizeof(long long)), "orr_debug_wave_times: alloc");
    HIPCHK(hipMemset(g_wave_times_dev, 0, (size_t)waves * 4 * sizeof(long long)), "orr_debug_wave_times: clear");
    g_wave_times_cap = waves;
    return 0;
  }
  if (out) HIPCHK(hipMemcpy(out, g_wave_times_dev, (size_t)waves * 4 * sizeof(long long), hipMemcpyDeviceToHost), "orr_debug_wave_times: read");
  return 0;
}
#endif
#ifdef ORR_PHASE_TIMERS
// development aid: read (and optionally clear) the per-phase cycle totals of the instrumented wave
int orr_debug_phase_cycles(long long* out40, int reset) {
  HIPCHK(hipDeviceSynchronize(), "orr_debug_phase_cycles: sync");
  HIPCHK(hipMemcpyFromSymbol(out40, HIP_SYMBOL(g_phase_cycles), kPhaseSlots * sizeof(long long)), "orr_debug_phase_cycles: read");
  if (reset) {
    long long z[kPhaseSlots] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z, sizeof(z)), "orr_debug_phase_cycles: clear");
  }
  return 0;
}
// development aid: the phase totals (kPhaseSlots words) of each of the first 2048 waves of the last step launch of the main unit's kernel
int orr_debug_wave_phases(long long* out, int waves) {
  HIPCHK(hipDeviceSynchronize(), "orr_debug_wave_phases: sync");
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_phases), (size_t)waves * 40 * sizeof(long long)), "orr_debug_wave_phases: read");
  return 0;
}
#endif

}  // extern "C"
