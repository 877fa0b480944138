// orr_task.h -- motion clips, imitation reward / observation / termination, sensors, reset (ImitationTask, sensors, Minitaur.reset)
// (device code of libopenroborl_hip.so, included by orr_env_kernels.h after orr_device.h; see DESIGN.md sections 3-5)
#pragma once

// ================================================================================================
// reference-motion sampling (task/motion_data.py:417-509,591-633,682-718)
// ================================================================================================
struct Sample {
  int f0, f1, count;
  float blend, phase;
};
__device__ __forceinline__ double clip_phase_d(const DevClip& c, double t) {  // motion_data.py:210-232
  double ph = t / c.dur_d;
  if (c.flags & ORR_CLIP_WRAP) ph -= floor(ph);
  else ph = fmin(fmax(ph, 0.0), 1.0);
  return ph;
}
__device__ __forceinline__ float clip_phase(const DevClip& c, double t) { return (float)clip_phase_d(c, t); }
__device__ __forceinline__ Sample clip_index(const DevClip& c, double t) {  // motion_data.py:234-253,682-718
  Sample s;
  const bool wrap = c.flags & ORR_CLIP_WRAP;
  s.count = (int)floor(t / c.dur_d);
  if (!wrap) s.count = s.count < 0 ? 0 : (s.count > 1 ? 1 : s.count);
  const double ph = clip_phase_d(c, t);
  s.phase = (float)ph;
  if (!wrap && t <= 0.0) { s.f0 = 0; s.f1 = 0; s.blend = 0.0f; }
  else if (!wrap && t >= c.dur_d) { s.f0 = c.F - 1; s.f1 = c.F - 1; s.blend = 0.0f; }
  else {
    s.f0 = (int)(ph * (c.F - 1));
    s.f0 = s.f0 > c.F - 1 ? c.F - 1 : s.f0;
    s.f1 = s.f0 + 1 < c.F - 1 ? s.f0 + 1 : c.F - 1;
    const double nt = ph * c.dur_d, t0 = s.f0 * c.dt_d, t1 = s.f1 * c.dt_d;
    s.blend = s.f1 == s.f0 ? 0.0f : (float)((nt - t0) / (t1 - t0));
  }
  return s;
}
__device__ static void cycle_offset(const DevClip& c, int count, float pos[3], float rot[4]) {  // motion_data.py:591-633
  pos[0] = pos[1] = pos[2] = 0.0f;
  if (c.flags & ORR_CLIP_CYCLE_POS) {
    if (!(c.flags & ORR_CLIP_CYCLE_ROT)) {
      pos[0] = count * c.cdp[0]; pos[1] = count * c.cdp[1]; pos[2] = count * c.cdp[2];
    } else {
      for (int i = 0; i < count; i++) {
        float r[4], o[3];
        q_about_z(i * c.cdh, r);
        qrot(c.cdp, r, o);
        pos[0] += o[0]; pos[1] += o[1]; pos[2] += o[2];
      }
    }
  }
  if (!(c.flags & ORR_CLIP_CYCLE_ROT)) { rot[0] = rot[1] = rot[2] = 0.0f; rot[3] = 1.0f; }
  else q_about_z(count * c.cdh, rot);
}

// Sample the active clip at up to 5 times (lane l < nt samples time t_l): frames are staged into LDS by
// coalesced row loads (lanes 0..18 read one 19-float frame row), then lanes 0..nt-1 blend serially.
// Result: S.ph.end.pose[l] = raw (no origin offset) pose; if with_vel, S.vel = raw frame velocity at time of lane 0.
// Warm-up poses (imitation_task.py:985-1009) are substituted where `warm` and -warmup <= t < 0.
// Two halves, so that the round trip of the frame loads can be covered by independent work of the caller: sample_poses_issue
// computes the frame indices and issues the loads (into registers), sample_poses_finish stages and blends them.
struct PoseLoads {
  float lo[11], hi[11], v0[2], v1[2];   // frame rows: word `lane` and, for lanes 0..2, word 16 + lane; frame velocities of lane 0's time
  Sample sm;
};
__device__ static void sample_poses_issue(const KParams& P, Shared& S, int lane, double t_lane, PoseLoads& L, int pt_slot = 32) {
  constexpr int nt = 5;   // update time + the four target times (compile-time: the staging arrays below must stay in registers)
  const DevClip& c = S.clip;
  const Sample sm = clip_index(c, lane < nt ? t_lane : 0.0);
  L.sm = sm;
  if (lane < nt) { S.ph.end.red[2 * lane] = __int_as_float(sm.f0); S.ph.end.red[2 * lane + 1] = __int_as_float(sm.f1); }
  WSYNC();
  PT(pt_slot);
  {
    // The clip pointers come out of a table, i.e. as generic pointers: loads through them would be FLAT instructions, which also
    // count on the LDS counter, so every LDS access in between would wait for the previous frame to arrive (13 serialised round
    // trips).  They point to global memory (orr_set_motion takes device pointers): say so, fetch all rows at once (frame row = 19
    // words: lane i and, for lanes 0..2, word 16 + i).
    typedef const float __attribute__((address_space(1))) * gptr;
    const gptr frames = (gptr)c.frames, vels = (gptr)c.vels;
    constexpr int kMaxE = 2 * nt;
    const int w1 = lane < 3 ? 16 + lane : lane;
#pragma unroll
    for (int e = 0; e < kMaxE; e++) {
      const int f = __float_as_int(S.ph.end.red[e]);
      L.lo[e] = frames[f * 19 + lane]; L.hi[e] = frames[f * 19 + w1];
    }
    L.lo[kMaxE] = frames[lane]; L.hi[kMaxE] = frames[w1];                       // frame 0 (warm-up heading)
    const int f0 = __float_as_int(S.ph.end.red[0]), f1 = __float_as_int(S.ph.end.red[1]);
    const int w2 = lane < 2 ? 16 + lane : lane;
    L.v0[0] = vels[f0 * 18 + lane]; L.v0[1] = vels[f0 * 18 + w2];
    L.v1[0] = vels[f1 * 18 + lane]; L.v1[1] = vels[f1 * 18 + w2];
  }
  WSYNC();   // red[] may be reused by the caller from here on
}
__device__ static void sample_poses_finish(const KParams& P, Shared& S, int lane, double t_lane, bool with_vel, const PoseLoads& L, int pt_slot = 32) {
  constexpr int nt = 5, kMaxE = 2 * nt;
  const DevClip& c = S.clip;
  const bool warm_ep = geti(S, O(WARMUP)) != 0;
  const Sample sm = L.sm;
#pragma unroll
  for (int e = 0; e <= kMaxE; e++) {
    S.ph.end.frames[e][lane] = L.lo[e];
    if (lane < 3) S.ph.end.frames[e][16 + lane] = L.hi[e];
  }
  if (with_vel) {
    S.ph.end.fvel[0][lane] = L.v0[0]; S.ph.end.fvel[1][lane] = L.v1[0];
    if (lane < 2) { S.ph.end.fvel[0][16 + lane] = L.v0[1]; S.ph.end.fvel[1][16 + lane] = L.v1[1]; }
  }
  WSYNC();
  PT(pt_slot + 1);
  if (lane < nt) {
    const bool warm_pose = warm_ep && t_lane >= -(double)P.cfg.warmup_time && t_lane < 0.0;
    float out[19];
    if (warm_pose) {
      // default pose rotated to the heading of frame(0) (imitation_task.py:985-1009, 1245-1252); warm-up episodes only (cold table)
      const ColdPtr mc = model_cold(P, geti(S, O(ROBOT_TYPE)));
      const float ipos[3] = {mc->init_pos[0], mc->init_pos[1], mc->init_pos[2]};
      const float* fr0 = S.ph.end.frames[10];
      float dr[4], pp[3], qq[4], q0[4] = {fr0[3], fr0[4], fr0[5], fr0[6]};
      const float dh = qheading(q0) - qheading(S.m.init_quat);
      q_about_z(dh, dr);
      qrot(ipos, dr, pp);
      qmul(dr, S.m.init_quat, qq);
      out[0] = pp[0]; out[1] = pp[1]; out[2] = pp[2];
      out[3] = qq[0]; out[4] = qq[1]; out[5] = qq[2]; out[6] = qq[3];
#pragma unroll
      for (int i = 0; i < 12; i++) out[7 + i] = mc->default_joints[i];
    } else {
      const float* a = S.ph.end.frames[2 * lane];
      const float* b = S.ph.end.frames[2 * lane + 1];
      const float bl = sm.blend;
#pragma unroll
      for (int k = 0; k < 3; k++) out[k] = (1.0f - bl) * a[k] + bl * b[k];
      float q[4];
      qslerp(a + 3, b + 3, bl, q);
      qstd(q);
#pragma unroll
      for (int k = 7; k < 19; k++) out[k] = (1.0f - bl) * a[k] + bl * b[k];
      float cp[3], cr[4], p[3], q2[4];
      cycle_offset(c, sm.count, cp, cr);
      qrot(out, cr, p);
      out[0] = p[0] + cp[0]; out[1] = p[1] + cp[1]; out[2] = p[2] + cp[2];
      qmul(cr, q, q2);
      qstd(q2);
      out[3] = q2[0]; out[4] = q2[1]; out[5] = q2[2]; out[6] = q2[3];
    }
#pragma unroll
    for (int k = 0; k < 19; k++) S.ph.end.pose[lane][k] = out[k];
    if (with_vel && lane == 0) {
      if (warm_pose) {
#pragma unroll
        for (int k = 0; k < 18; k++) S.ph.end.vel[k] = 0.0f;
      } else {
        float v[18], cp[3], cr[4], t3[3];
#pragma unroll
        for (int k = 0; k < 18; k++) v[k] = (1.0f - sm.blend) * S.ph.end.fvel[0][k] + sm.blend * S.ph.end.fvel[1][k];
        cycle_offset(c, sm.count, cp, cr);
        qrot(&v[0], cr, t3); v[0] = t3[0]; v[1] = t3[1]; v[2] = t3[2];
        qrot(&v[3], cr, t3); v[3] = t3[0]; v[4] = t3[1]; v[5] = t3[2];
#pragma unroll
        for (int k = 0; k < 18; k++) S.ph.end.vel[k] = v[k];
      }
    }
  }
  WSYNC();
}

// apply the origin offset (imitation_task.py:938-951) to S.ph.end.pose[l] in place (lane l < nt)
__device__ static void apply_origin(Shared& S, int lane, int nt) {
  if (lane < nt) {
    float qq[4], pp[3];
    qmul(&S.s[O(ORIGIN_ROT)], &S.ph.end.pose[lane][3], qq);
    qrot(&S.ph.end.pose[lane][0], &S.s[O(ORIGIN_ROT)], pp);
    S.ph.end.pose[lane][0] = pp[0] + S.s[O(ORIGIN_POS)]; S.ph.end.pose[lane][1] = pp[1] + S.s[O(ORIGIN_POS) + 1]; S.ph.end.pose[lane][2] = pp[2] + S.s[O(ORIGIN_POS) + 2];
    S.ph.end.pose[lane][3] = qq[0]; S.ph.end.pose[lane][4] = qq[1]; S.ph.end.pose[lane][5] = qq[2]; S.ph.end.pose[lane][6] = qq[3];
  }
  WSYNC();
}

__device__ __forceinline__ double motion_time(const KParams& P, const Shared& S) {  // imitation_task.py:831-848
  double t = geti(S, O(STATE_ACTION_COUNTER)) * S.clip.sim_dt_d + (double)S.s[O(TIME_OFFSET)];
  if (geti(S, O(WARMUP))) t -= (double)P.cfg.warmup_time;   // 0.25: exact in float32
  return t;
}

// The frame-step count of the lane's target time: lanes 1..4 get tar_frame_steps[0..3] (the other lanes get one of them and do not use
// it).  The four counts are kernel arguments.  Indexing them with the lane makes the compiler read the kernel-argument segment with a
// vector load - and so does a chain of selects over the four fields, which it folds back into a select of the byte offset followed by
// that load - whose wait (loads, stores and atomics share one in-order counter) also drains every store and atomic issued before it.
// Each count is therefore made opaque to the optimiser while it sits in its scalar register; the selects then stay register selects
// (tests/test_step_end_isa.py).
__device__ __forceinline__ int target_frame_steps(const orr_config& c, int lane) {
  int i0 = 0;
  asm("" : "+s"(i0));
  int s0 = c.tar_frame_steps[i0], s1 = c.tar_frame_steps[i0 + 1], s2 = c.tar_frame_steps[i0 + 2], s3 = c.tar_frame_steps[i0 + 3];
  asm("" : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3));
  const int k = lane - 1;
  return (k & 2) ? ((k & 1) ? s3 : s2) : ((k & 1) ? s1 : s0);
}

// Philox blocks of the task noise (orr_set_task_noise; below 2^30: a draw index is 4 * block + word, 32 bits)
constexpr uint32_t kNoiseResetBlock = 0x20000000u, kNoiseHeadingBlock = 0x30000000u;
// Philox blocks of the randomiser's four newer parameters (orr_set_randomizer): block 0x40000000 = base mass, global motor strength, the
// weakened leg, leg weaken's ratio; block 0x40000001 word 0 = single leg weaken
constexpr uint32_t kRandBlock = 0x40000000u;
// Philox blocks of the sensor noise (orr_set_sensor_noise): 0x10000000 + (i << 9) + (slot << 4) + lane, i = 0 for a reset of the episode,
// 1 + s for the step whose env-step counter before it is s.  Slots 0..16: the sub-steps' motor-angle readings (lane = motor; sub-step
// 2 slot: words 0, 1, sub-step 2 slot + 1: words 2, 3; z0 = the command clip's reading, z1 = the interpolation start's), 17: the sensor
// histories' readings (lane = column), 18: the filter history's initial value (lane = motor), 19: the target observation's rpy
constexpr uint32_t kSensorBlock = 0x10000000u, kSensorSlotHist = 17u, kSensorSlotFilter = 18u, kSensorSlotTarget = 19u;
__device__ __forceinline__ uint32_t sensor_block(uint32_t i, uint32_t slot, uint32_t lane) { return kSensorBlock + (i << 9) + (slot << 4) + lane; }
// the handle's three deviations, each the same in every lane (scalar registers from here on)
__device__ __forceinline__ SensorNoise load_sensor_noise(const KParams& P) {
  typedef const float __attribute__((address_space(1)))* gfp;
  const gfp sp = (gfp)&P.tab->sensor.motor_angle_std;
  static_assert(offsetof(orr_sensor_noise, base_rpy_std) == 12 && offsetof(orr_sensor_noise, base_rpy_rate_std) == 16, "words 0, 3, 4");
  SensorNoise SN;
  SN.a = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sp[0])));
  SN.r = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sp[3])));
  SN.d = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sp[4])));
  return SN;
}

// build the 76-d target observation into obs76 (LDS) from S.ph.end.pose[1..4] (already origin-offset) -- imitation_task.py:254-301.
// The control observation S.co must be current (it is after the last sub-step's ring push and after reset_robot_state's local blend).
// NOISE (the noise variants, orr_kernels_noise.hip): tar_obs_noise[0] of the reference (:273-275) - the heading the target frames are
// expressed in gets orr_task_noise::tar_heading_std times a normal from block 0x30000000 + noise_i of the stream (robot index, episode):
// noise_i = 0 for the observation of a reset, 1 + s for the step whose env-step counter before the step is s.  Both come from the
// caller's registers: the record's EP_STEP / EPISODE_IDX words are rewritten by lane 0 right before the calls
// SENS (the sensor variants, orr_kernels_sensor.hip; always with NOISE): the heading is formed from get_base_rpy's noisy reading
// (minitaur.py:630-638) - pitch and yaw each get SN.r times a normal of slot 19 of the same (episode, noise_i); roll's draw is unused
template <bool NOISE = false, bool SENS = false>
__device__ static void target_obs(const KParams& P, const float* rec, Shared& S, int lane, float* obs76, uint32_t episode = 0u, uint32_t noise_i = 0u,
                                  const SensorNoise& SN = SensorNoise{}) {
  if (lane >= 1 && lane <= 4) {
    float rpy[3];
    euler_from_quat(&S.co[12], rpy);
    if constexpr (SENS) {
      if (SN.r > 0.0f) {   // wave-uniform
        float u4[4], zr, zp, zy, zu;
        philox_block(P.cfg.seed, (uint32_t)geti(S, O(ROBOT_INDEX)), episode, sensor_block(noise_i, kSensorSlotTarget, 0u), u4);
        normal_pair(u4[0], u4[1], &zr, &zp);
        normal_pair(u4[2], u4[3], &zy, &zu);
        rpy[1] = fmaf(SN.r, zp, rpy[1]);
        rpy[2] = fmaf(SN.r, zy, rpy[2]);
      }
    }
    // robot.get_base_orientation (minitaur.py:630-638) = quaternion of the delayed rpy; its heading is the
    // direction of the rotated x axis = atan2(sin(yaw) cos(pitch), cos(yaw) cos(pitch))
    float sy, cy, spch, cpch;
    joint_sincos(rpy[1], &spch, &cpch);
    joint_sincos(rpy[2], &sy, &cy);
    float heading = atan2_bf(sy * cpch, cy * cpch);
    if constexpr (NOISE) {   // lanes 1..4 evaluate the same draw: one lane's cost for the wave
      typedef const float __attribute__((address_space(1)))* gfp;
      const float sigma = ((gfp)&P.tab->noise.tar_heading_std)[0];
      float u4[4], z0, z1;
      philox_block(P.cfg.seed, (uint32_t)geti(S, O(ROBOT_INDEX)), episode, kNoiseHeadingBlock + noise_i, u4);
      normal_pair(u4[0], u4[1], &z0, &z1);
      heading = fmaf(sigma, z0, heading);     // sigma = 0: the heading itself (z0 is finite)
    }
    float ih[4], p[3], pr[3], q[4];
    q_about_z(-heading, ih);
    const float* pose = S.ph.end.pose[lane];
    p[0] = pose[0] - S.s[O(REF_POSE)]; p[1] = pose[1] - S.s[O(REF_POSE) + 1]; p[2] = pose[2] - S.s[O(REF_POSE) + 2];
    qrot(p, ih, pr);
    qmul(ih, pose + 3, q);
    qstd(q);
    float* o = obs76 + (lane - 1) * 19;
    o[0] = pr[0]; o[1] = pr[1]; o[2] = pr[2]; o[3] = q[0]; o[4] = q[1]; o[5] = q[2]; o[6] = q[3];
#pragma unroll
    for (int k = 7; k < 19; k++) o[k] = pose[k];
  }
  WSYNC();
}

// forward kinematics of one leg's two end-effector link COMs (lower leg, toe) -- getLinkState in
// imitation_task.py:441-446; link set minitaur.py:842-844
__device__ static void leg_end_effectors(const Shared& S, const float pos[3], const float quat[4], const float* qj, int leg,
                                         float lower[3], float toe[3]) {
  float qi[4], qrel[4], R[9], o[3] = {pos[0], pos[1], pos[2]};
  qinv(S.m.init_quat, qi);
  qmul(quat, qi, qrel);
  q_to_mat(qrel, R);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int j = 3 * leg + k;
    float t[3];
    mv3(R, S.m.joint_pos[j], t);
    o[0] += t[0]; o[1] += t[1]; o[2] += t[2];
    const float a = S.m.jdir[j] * (qj[j] - S.m.joff[j]);
    float sn, cs;
    joint_sincos(a, &sn, &cs);
#pragma unroll
    for (int i = 0; i < 3; i++) {  // R <- R Rj (joint k = 0 turns about x, k = 1, 2 about y)
      const float p0 = R[3 * i], p1 = R[3 * i + 1], p2 = R[3 * i + 2];
      if (k == 0) { R[3 * i + 1] = cs * p1 + sn * p2; R[3 * i + 2] = -sn * p1 + cs * p2; }
      else { R[3 * i] = cs * p0 - sn * p2; R[3 * i + 2] = sn * p0 + cs * p2; }
    }
  }
  float t[3];
  mv3(R, S.m.lower_com[leg], t); lower[0] = o[0] + t[0]; lower[1] = o[1] + t[1]; lower[2] = o[2] + t[2];
  mv3(R, S.m.toe_pos[leg], t); toe[0] = o[0] + t[0]; toe[1] = o[1] + t[1]; toe[2] = o[2] + t[2];
}

__device__ __forceinline__ void task_heading_rot(const Shared& S, const float q[4], float out[4]) {  // imitation_task.py:1168-1189
  float dc[4], rel[4];
  qconj(S.m.init_quat, dc);
  qmul(q, dc, rel);
  q_about_z(qheading(rel), out);
}
__device__ __forceinline__ float task_heading(const Shared& S, const float q[4]) {  // _calc_heading, imitation_task.py:1143-1166
  float dc[4], rel[4];
  qconj(S.m.init_quat, dc);
  qmul(q, dc, rel);
  return qheading(rel);
}

// the motion time of the next clip change (_reset_clip_change_time, imitation_task.py:1057-1069): t + U(tmin, tmax) in float64 as the
// reference computes it (numpy's uniform: low + (high - low) u), rounded to the record's float32; +inf where switching is off
__device__ __forceinline__ float clip_change_time(double t, float tmin, float tmax, float u) {
  if (!(tmax < INFINITY)) return INFINITY;   // orr_set_clip_switch: both bounds finite, or both +inf
  return (float)(t + ((double)tmin + ((double)tmax - (double)tmin) * (double)u));
}

// ImitationTask.reward (imitation_task.py:341-516); every lane returns the same value
// eff_replay (parity replay only, else NULL): [2][8][3] link positions that replace the forward kinematics
// terms (TERMS, the terms variant, only; else NULL): gets the five unweighted terms exp(-scale_k err_k) in reward_w's order - pose, velocity, end
// effector, root pose, root velocity (_calc_reward_pose .. _calc_reward_root_velocity, :358-516) - and the reward is summed from them
template <bool TERMS = false>
__device__ static float calc_reward(const KParams& P, Shared& S, int lane, const float* eff_replay = nullptr, float* terms = nullptr) {
  const float* rp = &S.s[O(REF_POSE)];
  const float* rv = &S.s[O(REF_VEL)];
  if (lane < 8) {
    const int leg = lane & 3, which = lane >> 2;  // 0 sim, 1 ref
    float lower[3], toe[3];
    if (which == 0) leg_end_effectors(S, &S.s[O(POS)], &S.s[O(QUAT)], &S.s[O(Q)], leg, lower, toe);
    else leg_end_effectors(S, rp, rp + 3, rp + 7, leg, lower, toe);
#pragma unroll
    for (int i = 0; i < 3; i++) { S.ph.end.ee[which][2 * leg][i] = lower[i]; S.ph.end.ee[which][2 * leg + 1][i] = toe[i]; }
  }
  if (eff_replay) {
    WSYNC();
    for (int i = lane; i < 48; i += kLanes) (&S.ph.end.ee[0][0][0])[i] = eff_replay[i];
  }
  WSYNC();
  const orr_config& c = P.cfg;
  float pose_err = 0.0f, vel_err = 0.0f, ee_err = 0.0f;
#pragma unroll
  for (int j = 0; j < 12; j++) {
    float d = rp[7 + j] - S.s[O(Q) + j];
    pose_err += d * d;
    d = rv[6 + j] - S.s[O(QD) + j];
    vel_err += d * d;
  }
  {
    float hr[4], hs[4], ihr[4], ihs[4];
    task_heading_rot(S, rp + 3, hr);
    task_heading_rot(S, &S.s[O(QUAT)], hs);
    qconj(hr, ihr);
    qconj(hs, ihs);
    // each of lanes 0..7 handles one end effector, then an 8-lane sum
    float e = 0.0f;
    if (lane < 8) {
      float a[3], b[3], ar[3], br[3];
#pragma unroll
      for (int k = 0; k < 3; k++) { a[k] = S.ph.end.ee[1][lane][k] - rp[k]; b[k] = S.ph.end.ee[0][lane][k] - S.s[O(POS) + k]; }
      qrot(a, ihr, ar);
      qrot(b, ihs, br);
      const float dh = S.ph.end.ee[1][lane][2] - S.ph.end.ee[0][lane][2];
      e = (ar[0] - br[0]) * (ar[0] - br[0]) + (ar[1] - br[1]) * (ar[1] - br[1]) + c.reward_scale[3] * dh * dh;
    }
    S.ph.end.red[lane] = e;
    WSYNC();
#pragma unroll
    for (int k = 0; k < 8; k++) ee_err += S.ph.end.red[k];
  }
  float root_pose_err, root_vel_err;
  {
    float pe = 0.0f, qc[4], dq[4];
#pragma unroll
    for (int k = 0; k < 3; k++) { float d = rp[k] - S.s[O(POS) + k]; pe += d * d; }
    qconj(&S.s[O(QUAT)], qc);
    qmul(rp + 3, qc, dq);
    const float ang = q_norm_angle(dq);
    root_pose_err = pe + 0.5f * ang * ang;
    float ve = 0.0f, we = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      float d = rv[k] - S.s[O(LINVEL) + k]; ve += d * d;
      d = rv[3 + k] - S.s[O(ANGVEL) + k]; we += d * d;
    }
    root_vel_err = ve + 0.1f * we;
  }
  if constexpr (TERMS) {
    terms[0] = expf(-c.reward_scale[0] * pose_err); terms[1] = expf(-c.reward_scale[1] * vel_err); terms[2] = expf(-c.reward_scale[2] * ee_err);
    terms[3] = expf(-c.reward_scale[4] * root_pose_err); terms[4] = expf(-c.reward_scale[5] * root_vel_err);
    const float r = c.reward_w[0] * terms[0] + c.reward_w[1] * terms[1] + c.reward_w[2] * terms[2] + c.reward_w[3] * terms[3] + c.reward_w[4] * terms[4];
    WSYNC();
    return r;
  }
  const float r = c.reward_w[0] * expf(-c.reward_scale[0] * pose_err) + c.reward_w[1] * expf(-c.reward_scale[1] * vel_err) +
                  c.reward_w[2] * expf(-c.reward_scale[2] * ee_err) + c.reward_w[3] * expf(-c.reward_scale[4] * root_pose_err) +
                  c.reward_w[4] * expf(-c.reward_scale[5] * root_vel_err);
  WSYNC();
  return r;
}

__device__ __forceinline__ int time_limit(const orr_config& c, long long total) {  // wrapper_env.py:151-159
  if (!(c.flags & ORR_FLAG_CURRICULUM) || c.curriculum_steps <= 0) return c.ep_len_end;
  double t = (double)total / (double)c.curriculum_steps;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  t = t * t * t;
  return (int)((1.0 - t) * c.ep_len_start + t * c.ep_len_end);
}

// current sensor readings (robot_sensors.py:74-83,153-190) from S.co -> push into the 3-deep histories
__device__ static void sensors_push(Shared& S, int lane, bool fill_all) {
  float rpy[3];
  euler_from_quat(&S.co[12], rpy);
  // 28 history columns: 0..11 motor angle k, 12..15 IMU channel, 16..27 last action; a lane owns columns lane, lane+kLanes
  constexpr int kCols = (28 + kLanes - 1) / kLanes;
  float newest[kCols], h0[kCols], h1[kCols];
  int base[kCols], w[kCols], kk[kCols];
#pragma unroll
  for (int c = 0; c < kCols; c++) {
    const int col = lane + c * kLanes;
    base[c] = 0; w[c] = 0; kk[c] = 0; newest[c] = 0.0f; h0[c] = 0.0f; h1[c] = 0.0f;
    if (col < 12) { base[c] = O(MOTORANG_HIST); w[c] = 12; kk[c] = col; newest[c] = map_pi(S.co[col]); }
    else if (col < 16) { base[c] = O(IMU_HIST); w[c] = 4; kk[c] = col - 12; newest[c] = kk[c] == 0 ? rpy[0] : (kk[c] == 1 ? rpy[1] : (kk[c] == 2 ? S.co[16] : S.co[17])); }
    else if (col < 28) { base[c] = O(LASTACT_HIST); w[c] = 12; kk[c] = col - 16; newest[c] = S.s[O(LAST_ACTION) + kk[c]]; }
    if (col < 28) { h0[c] = S.s[base[c] + kk[c]]; h1[c] = S.s[base[c] + w[c] + kk[c]]; }
  }
  WSYNC();
#pragma unroll
  for (int c = 0; c < kCols; c++) {
    if (lane + c * kLanes < 28) {
      S.s[base[c] + kk[c]] = newest[c];
      S.s[base[c] + w[c] + kk[c]] = fill_all ? newest[c] : h0[c];
      S.s[base[c] + 2 * w[c] + kk[c]] = fill_all ? newest[c] : h1[c];
    }
  }
  WSYNC();
}

// sensors_push of the sensor variants (orr_kernels_sensor.hip; a function of its own: the other variants keep theirs as it is): the motor-angle columns read map_pi(angle + SN.a z), roll and pitch rpy + SN.r z, the two rates rate +
// SN.d z, z from slot 17 of (episode, noise_i), lane = column (a lane's first column).  A step takes z0 of the pair (word 0, word 1).  A
// reset (fill_all) takes three separate readings (HistoricSensorWrapper.on_reset, sensor_wrappers.py:122-129) - z0, z1 of that pair, then
// z0 of the pair (word 2, word 3) - and the first one ends up as the oldest entry.  A deviation of 0 passes the reading's bits
__device__ static void sensors_push_noisy(Shared& S, int lane, bool fill_all, const SensorNoise& SN, unsigned long long seed, uint32_t episode,
                                          uint32_t noise_i) {
  constexpr bool SENS = true;
  float rpy[3];
  euler_from_quat(&S.co[12], rpy);
  static_assert(!SENS || kLanes == 16, "SENS: the sixteen noisy columns are the lanes' first columns");
  float sg = 0.0f, zs[3] = {0.0f, 0.0f, 0.0f};
  if constexpr (SENS) {
    if (SN.a > 0.0f || SN.r > 0.0f || SN.d > 0.0f) {   // wave-uniform
      sg = lane < 12 ? SN.a : (lane < 14 ? SN.r : SN.d);
      float u4[4], zu;
      philox_block(seed, (uint32_t)geti(S, O(ROBOT_INDEX)), episode, sensor_block(noise_i, kSensorSlotHist, (uint32_t)lane), u4);
      normal_pair(u4[0], u4[1], &zs[0], &zs[1]);
      if (fill_all) normal_pair(u4[2], u4[3], &zs[2], &zu);
    }
  }
  // 28 history columns: 0..11 motor angle k, 12..15 IMU channel, 16..27 last action; a lane owns columns lane, lane+kLanes
  constexpr int kCols = (28 + kLanes - 1) / kLanes;
  float newest[kCols], h0[kCols], h1[kCols];
  float rd1 = 0.0f, rd2 = 0.0f;   // SENS: the second and third reading of a reset, first column
  int base[kCols], w[kCols], kk[kCols];
#pragma unroll
  for (int c = 0; c < kCols; c++) {
    const int col = lane + c * kLanes;
    base[c] = 0; w[c] = 0; kk[c] = 0; newest[c] = 0.0f; h0[c] = 0.0f; h1[c] = 0.0f;
    if (col < 12) { base[c] = O(MOTORANG_HIST); w[c] = 12; kk[c] = col; newest[c] = map_pi(S.co[col]); }
    else if (col < 16) { base[c] = O(IMU_HIST); w[c] = 4; kk[c] = col - 12; newest[c] = kk[c] == 0 ? rpy[0] : (kk[c] == 1 ? rpy[1] : (kk[c] == 2 ? S.co[16] : S.co[17])); }
    else if (col < 28) { base[c] = O(LASTACT_HIST); w[c] = 12; kk[c] = col - 16; newest[c] = S.s[O(LAST_ACTION) + kk[c]]; }
    if constexpr (SENS) {
      if (c == 0) {
        rd1 = rd2 = newest[0];
        if (sg > 0.0f) {
          const float x = lane < 12 ? S.co[lane] : newest[0];
          const float r0 = fmaf(sg, zs[0], x), r1 = fmaf(sg, zs[1], x), r2 = fmaf(sg, zs[2], x);
          newest[0] = lane < 12 ? map_pi(r0) : r0;
          rd1 = lane < 12 ? map_pi(r1) : r1;
          rd2 = lane < 12 ? map_pi(r2) : r2;
        }
      }
    }
    if (col < 28) { h0[c] = S.s[base[c] + kk[c]]; h1[c] = S.s[base[c] + w[c] + kk[c]]; }
  }
  WSYNC();
#pragma unroll
  for (int c = 0; c < kCols; c++) {
    if (lane + c * kLanes < 28) {
      if (SENS && c == 0 && fill_all) {   // three readings: newest[0] was the first
        S.s[base[c] + kk[c]] = rd2;
        S.s[base[c] + w[c] + kk[c]] = rd1;
        S.s[base[c] + 2 * w[c] + kk[c]] = newest[c];
        continue;
      }
      S.s[base[c] + kk[c]] = newest[c];
      S.s[base[c] + w[c] + kk[c]] = fill_all ? newest[c] : h0[c];
      S.s[base[c] + 2 * w[c] + kk[c]] = fill_all ? newest[c] : h1[c];
    }
  }
  WSYNC();
}

// The clip draw of the CLIPS variants, at a reset (draw 28) and at a mid-episode switch (draw 32 + 4 s): lane l of the robot holds entry
// l of its type's clip set and the entry's interval [cum[l], cum[l + 1]) of the 24-bit thresholds (DevTables::clip_cum), and the entry
// whose interval holds m, the draw's 24-bit integer, is the one drawn.  clip_draw_issue starts the loads (global_load: nothing waits
// for them until clip_drawn reads them).  The uniform thresholds ceil(k 2^24 / n) that orr_set_clip_set writes pick (m n) >> 24.
struct ClipDraw {
  int set_id = 0, set_n = 0;
  uint32_t lo = 0, hi = 0;
};
__device__ __forceinline__ ClipDraw clip_draw_issue(const KParams& P, int type, int lane) {
  static_assert(ORR_MAX_CLIPS == kLanes, "one clip-set entry per lane");
  typedef const int __attribute__((address_space(1)))* gip;
  typedef const unsigned int __attribute__((address_space(1)))* gup;
  ClipDraw d;
  d.set_id = ((gip)&P.tab->clip_set[type][0])[lane];
  d.set_n = ((gip)&P.tab->clip_set_n[0])[type];
  d.lo = ((gup)&P.tab->clip_cum[type][0])[lane];
  d.hi = ((gup)&P.tab->clip_cum[type][0])[lane + 1];
  return d;
}
// -> this lane's entry is the one drawn (one lane of the robot at most; none for a type without a set: it keeps its CLIP_ID)
__device__ __forceinline__ bool clip_drawn(const ClipDraw& d, uint32_t m, int lane) { return lane < d.set_n && d.lo <= m && m < d.hi; }

// ================================================================================================
// reset of one robot (wrapper_env.py:87-107 -> quadruped_gym_env.py:63-104 -> minitaur.py:232-278 ->
// imitation_task.py:166-199); SURVEY.md Appendix A.2.
// ================================================================================================
// uni_replay (parity replay only, else NULL): 28 draws in [0, 1) that replace the Philox stream
// CLIPS (the multi-clip variants, orr_kernels_multiclip.hip): the episode's clip is drawn from the robot type's clip set (DevTables::clip_set)
// by the type's thresholds (DevTables::clip_cum; clip_draw_issue / clip_drawn above) with draw 28 (Philox block 7, word 0) before anything reads the clip, and CLIP_ID / S.clip hold it from then on; the record's
// CLIP_CHANGE_TIME (behind the ring, in memory: store_reset_extras) gets the episode's first clip change, draw 29 (orr_set_clip_switch)
// RC: the lane's cold-table constants (load_reset_const; the step kernel issues those loads right past its sub-steps)
// NOISE (the noise variants, orr_kernels_noise.hip; always with CLIPS): perturb_init_state_prob / _apply_state_perturb of the reference
// (:192-197, 1195-1243) - with probability orr_task_noise::perturb_init_state_prob stage 6 puts the robot on a Gaussian-perturbed copy
// of the reference state (draw rule: include/openroborl_hip.h, orr_set_task_noise) - and the noisy heading of target_obs<true>
// Two parts.  reset_robot_state puts the robot's LDS image on the new episode: everything but the observation.  It issues every load
// first and STORES NOTHING - the ring entries #1 / #2 of the new episode stay in LDS (reset_entry1 / reset_entry2) and the CLIPS
// variants' change time comes back in *clip_change; the caller stores them with store_reset_extras at the end of its kernel, with the
// record.  build_obs then writes the observation; the step kernel calls it once for all its robots, reset or not.  -> the new episode index
__device__ __forceinline__ float* reset_entry1(Shared& S) { return S.ph.end.red; }        // 20 words each; no step-end code past the reset
__device__ __forceinline__ float* reset_entry2(Shared& S) { return S.ph.end.red + 56; }   // touches red[]
// SENS (the sensor variants, orr_kernels_sensor.hip; always with NOISE): stage 3 fills the sensor histories with three separate noisy
// readings (sensors_push_noisy; i = 0 of the new episode's stream)
// RAND (the randomiser variants, orr_kernels_randomizer.hip; always with SENS): stage 4b is table-driven (orr_set_randomizer: ten
// parameters, each enabled or not, with its own range) and controllable (orr_bind_randomizer_params: RR->row is the robot's row of the
// params buffer; the lane's two words of the new episode's row come back in RR->a / RR->b for the caller to store with the record, or,
// suspended, the row is loaded here with the reset's first loads and applied instead of the draws)
template <bool CLIPS = false, bool NOISE = false, bool SENS = false, bool RAND = false>
__device__ static uint32_t reset_robot_state(const KParams& P, Shared& S, int lane, long long total_step_count, const ResetConst& RC,
                                             float* clip_change, const float* uni_replay = nullptr, const SensorNoise& SN = SensorNoise{},
                                             RandRow* RR = nullptr) {
  const orr_config& c = P.cfg;
  // every reset starts a new episode = a new RNG stream (robot, episode)
  const uint32_t robot = (uint32_t)geti(S, O(ROBOT_INDEX)), ep = (uint32_t)geti(S, O(EPISODE_IDX)) + 1u;
  WSYNC();
  if (lane == 0) {
    seti(S, O(EPISODE_IDX), (int)ep);
    seti(S, O(STATE_ACTION_COUNTER), 0);    // of stage 1-2 below: the start time (motion_time) reads it
  }
  PT(16);
  // Order of the stages below: what needs global memory is started first (the episode's draws fix the start time, hence the clip
  // frames), the stages that need nothing from memory run while those loads are in flight, then comes the ONE wait for the frames.
  // 4a. all 28 draws of the episode (0..25 randomiser, 26 ref-state-init, 27 time offset) = 7 Philox blocks: lane b < 7 evaluates
  // block b once and parks its four numbers in LDS
  float* draws = S.ph.end.red + 24;    // 28 words (CLIPS: 32, block 7 in red[52..55], free until ring entry #2 takes red[56..75])
  static_assert(kLanes == 16, "reset_robot_state / the pose sampler assume 16 lanes per robot");
  ClipDraw cdraw;
  float sw_min = 0.0f, sw_max = 0.0f;
  if constexpr (CLIPS) {   // the type's clip set, one id and one threshold interval per lane, and switch interval, in flight while the Philox blocks are evaluated
    typedef const float __attribute__((address_space(1)))* gfp;
    const int type = geti(S, O(ROBOT_TYPE));
    cdraw = clip_draw_issue(P, type, lane);
    sw_min = ((gfp)&P.tab->clip_switch[type][0])[0];
    sw_max = ((gfp)&P.tab->clip_switch[type][0])[1];
  }
  // RAND: the handle's table - the lane's own parameter (that of draw `lane`, the existing loop's mapping) and the five that every
  // lane needs (motor strength, global motor strength, leg weaken, single leg weaken for the STRENGTH word that lanes 0..11 own, base
  // mass for lane 12's MASS_RATIO[0]) - and, suspended, the robot's row: all in flight while the Philox blocks are evaluated.  The two
  // new blocks' words park in xb[0..7] = ee[36..43], behind the noise stage's 36 words (ee: see nz below)
  float* xb = &S.ph.end.ee[0][0][0] + 36;
  int rn_en = 0, rn_en_u[5] = {0, 0, 0, 0, 0};
  float rn_lo = 0.0f, rn_hi = 0.0f, rn_lo_u[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, rn_hi_u[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float row_a = 0.0f, row_ms = 0.0f, row_x[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // suspended: row words lane, 14 + lane, 26..30
  constexpr int kRandU[5] = {ORR_RAND_MOTOR_STRENGTH, ORR_RAND_GLOBAL_MOTOR_STRENGTH, ORR_RAND_LEG_WEAKEN, ORR_RAND_SINGLE_LEG_WEAKEN, ORR_RAND_BASE_MASS};
  if constexpr (RAND) {
    static_assert(sizeof(S.ph.end.ee) >= 44 * sizeof(float), "36 words of the noise stage + two blocks");
    typedef const int __attribute__((address_space(1)))* gip;
    typedef const float __attribute__((address_space(1)))* gfp;
    const gip en = (gip)&P.tab->rnd.enabled[0];
    const gfp lo = (gfp)&P.tab->rnd.lo[0], hi = (gfp)&P.tab->rnd.hi[0];
    const int pa = lane < 2 ? ORR_RAND_INERTIA : (lane < 10 ? ORR_RAND_JOINT_FRICTION : (lane == 10 ? ORR_RAND_LATENCY : (lane == 11 ? ORR_RAND_LATERAL_FRICTION
                   : (lane < 14 ? ORR_RAND_MASS : ORR_RAND_MOTOR_STRENGTH))));
    rn_en = en[pa]; rn_lo = lo[pa]; rn_hi = hi[pa];
#pragma unroll
    for (int k = 0; k < 5; k++) { rn_en_u[k] = en[kRandU[k]]; rn_lo_u[k] = lo[kRandU[k]]; rn_hi_u[k] = hi[kRandU[k]]; }
    if (RR->suspend) {   // wave-uniform.  Words 14 + lane of lanes 12..15 are not motor-strength draws: they repeat word 31
      const gfp r = (gfp)RR->row;
      row_a = r[lane]; row_ms = r[lane < 12 ? 14 + lane : ORR_RAND_ROW - 1];
#pragma unroll
      for (int k = 0; k < 5; k++) row_x[k] = r[26 + k];
    }
  }
  if constexpr (RAND) {   // blocks 0..7 as below and, in lanes 8 and 9, blocks 0x40000000 and 0x40000001 (always from Philox)
    static_assert(CLIPS, "the randomiser variants hold the clip-set code");
    if (lane < 10) {
      float u4[4];
      if (uni_replay && lane < 7) { u4[0] = uni_replay[4 * lane]; u4[1] = uni_replay[4 * lane + 1]; u4[2] = uni_replay[4 * lane + 2]; u4[3] = uni_replay[4 * lane + 3]; }
      else philox_block(c.seed, robot, ep, lane < 8 ? (uint32_t)lane : kRandBlock + (uint32_t)(lane - 8), u4);
      float* dst = lane < 8 ? draws + 4 * lane : xb + 4 * (lane - 8);
      dst[0] = u4[0]; dst[1] = u4[1]; dst[2] = u4[2]; dst[3] = u4[3];
    }
  } else if (lane < (CLIPS ? 8 : 7)) {
    float u4[4];
    if (uni_replay && (!CLIPS || lane < 7)) { u4[0] = uni_replay[4 * lane]; u4[1] = uni_replay[4 * lane + 1]; u4[2] = uni_replay[4 * lane + 2]; u4[3] = uni_replay[4 * lane + 3]; }
    else philox_block(c.seed, robot, ep, (uint32_t)lane, u4);
    draws[4 * lane] = u4[0]; draws[4 * lane + 1] = u4[1]; draws[4 * lane + 2] = u4[2]; draws[4 * lane + 3] = u4[3];
  }
  WSYNC();
  float u_change = 0.0f;   // CLIPS: draw 29, the first clip change (red[] is reused before it is needed)
  if constexpr (CLIPS) {
    // draw 28 -> the entry k with cum[k] <= m < cum[k + 1], m = its 24-bit integer (u = m / 2^24 exactly): integer arithmetic; with the
    // uniform thresholds k = (m n) >> 24.  The lane that holds set[k] writes CLIP_ID; then the clip header is staged again, one word per
    // lane (as load_robot does)
    u_change = draws[29];
    const uint32_t m = (uint32_t)(draws[28] * 16777216.0f);
    if (clip_drawn(cdraw, m, lane)) seti(S, O(CLIP_ID), cdraw.set_id);
    WSYNC();
    const unsigned int* cg = reinterpret_cast<const unsigned int*>(&P.tab->clip[geti(S, O(CLIP_ID))]);
    unsigned int* cl = reinterpret_cast<unsigned int*>(&S.clip);
    if (lane < (int)(sizeof(DevClip) / 4)) cl[lane] = cg[lane];
    WSYNC();
  }
  // NOISE: the 36 uniforms U(k) of blocks 0x20000000 .. 0x20000008 (lane b < 9 evaluates block b) and the 32 normals made of them
  // (lane j: pair j of (U(4 + 2j), U(5 + 2j)), written over its own two uniforms) live in nz[0..35] = U(0..3), z0..z31 until stage 6.
  // Their home is the end-effector buffer of the reward (StepEndBuf::ee, 48 words): only calc_reward touches it, no reset stage does,
  // and in the step kernel the reward of the step is done before the auto-reset begins.  (red[] is full: draws in red[24..55], the
  // ring entries in red[0..19] and red[56..75]; frames / pose / vel are written by stages 5a-5b and read by stage 6.)
  float* nz = &S.ph.end.ee[0][0][0];
  float n_prob = 0.0f, n_pos = 0.0f, n_rot = 0.0f, n_jp = 0.0f, n_vel = 0.0f, n_ang = 0.0f, n_jv = 0.0f;
  if constexpr (NOISE) {
    static_assert(sizeof(S.ph.end.ee) >= 36 * sizeof(float), "U(0..3) + 32 normals");
    typedef const float __attribute__((address_space(1)))* gfp;
    const gfp ns = (gfp)&P.tab->noise.perturb_init_state_prob;     // the handle's setting, in flight while the blocks are evaluated
    n_prob = ns[0]; n_pos = ns[1]; n_rot = ns[2]; n_jp = ns[3]; n_vel = ns[4]; n_ang = ns[5]; n_jv = ns[6];
    if (lane < 9) {
      float u4[4];
      philox_block(c.seed, robot, ep, kNoiseResetBlock + (uint32_t)lane, u4);
      nz[4 * lane] = u4[0]; nz[4 * lane + 1] = u4[1]; nz[4 * lane + 2] = u4[2]; nz[4 * lane + 3] = u4[3];
    }
    WSYNC();
    float z0, z1;
    normal_pair(nz[4 + 2 * lane], nz[5 + 2 * lane], &z0, &z1);
    WSYNC();
    nz[4 + 2 * lane] = z0; nz[5 + 2 * lane] = z1;
    WSYNC();
  }
  PT(24);
  // 5a. task reset (imitation_task.py:183-199, 694-732, 1103-1110): start time -> frame loads issued
  const DevClip& clip = S.clip;
  {
    const float u1 = draws[26], u2 = draws[27];
    const bool ref_init = u1 < c.ref_state_init_prob;
    const bool warm = (!ref_init) && c.warmup_time > 0.0f;
    if (lane == 0) {
      seti(S, O(WARMUP), warm ? 1 : 0);
      S.s[O(TIME_OFFSET)] = warm ? u2 * c.warmup_time : u2 * (float)clip.dur_d;
      S.s[O(ORIGIN_POS)] = 0.0f; S.s[O(ORIGIN_POS) + 1] = 0.0f; S.s[O(ORIGIN_POS) + 2] = 0.0f;
      S.s[O(ORIGIN_ROT)] = 0.0f; S.s[O(ORIGIN_ROT) + 1] = 0.0f; S.s[O(ORIGIN_ROT) + 2] = 0.0f; S.s[O(ORIGIN_ROT) + 3] = 1.0f;
    }
    WSYNC();
  }
  const double t = motion_time(P, S);
  const double step_dt = S.clip.sim_dt_d * c.action_repeat;
  double tl = t;
  if (lane >= 1 && lane <= 4) tl = t + target_frame_steps(c, lane) * step_dt;   // lanes 1..4: the four target times
  PT(20);
  PoseLoads PL;
  sample_poses_issue(P, S, lane, tl, PL, 26);     // uses red[0..9] until it returns
  PT(19);
  // 1-2. default pose at the grid slot, counters, ring, filter (minitaur.py:246-268, 465-483).  The per-motor reset constants are the
  // caller's (RC), like the initial base position
  const int rj = RC.j;
  const float r_q0 = RC.init + RC.off, r_p0 = RC.p0;
  if (lane < 3) {
    S.s[O(POS) + lane] = r_p0 + (lane < 2 ? S.s[O(GRID_OFFSET) + lane] : 0.0f);
    S.s[O(LINVEL) + lane] = 0.0f; S.s[O(ANGVEL) + lane] = 0.0f;
  }
  if (lane < 4) S.s[O(QUAT) + lane] = S.m.init_quat[lane];
  if (lane < 12) {
    const int j = rj;
    S.s[O(Q) + j] = r_q0;  // no direction factor (minitaur.py:481)
    S.s[O(QD) + j] = 0.0f;
    S.s[O(LAST_ACTION) + lane] = 0.0f; S.s[O(ACTION) + lane] = 0.0f; S.s[O(FILTER_ACTION) + lane] = 0.0f; S.s[O(LAMBDA) + lane] = 0.0f;
    S.s[O(XHIST) + lane] = 0.0f; S.s[O(XHIST) + 12 + lane] = 0.0f; S.s[O(YHIST) + lane] = 0.0f; S.s[O(YHIST) + 12 + lane] = 0.0f;
  }
  if (lane == 0) {
    seti(S, O(RING_LEN), 0); seti(S, O(RING_HEAD), ORR_RING_DEPTH - 1);
    seti(S, O(STEP_COUNTER), 0); seti(S, O(FILTER_VALID), 0);     // (STATE_ACTION_COUNTER: at the top)
    seti(S, O(EP_STEP), 0);   // DONE_REASON keeps the reason the PREVIOUS episode ended with until the next step overwrites it (env.stats())
    S.s[O(EP_RETURN)] = 0.0f;
  }
  WSYNC();
  // ring entries #1 and #2 of the new episode are kept (LDS) so that the control observations of the reset are blended from them
  // directly, and stored by the caller at the end of its kernel (ring slots 0 and 1: the ring restarts behind its last slot)
  float* e1 = reset_entry1(S);
  receive_obs(S, lane, RC, e1);  // ring entry #1
  // 3. sensor histories <- 3 copies of the current readings (minitaur.py:270-271; sensor_wrappers.py:122-129)
  PT(17);
  WSYNC();
  for (int i = lane; i < 19; i += kLanes) S.co[i] = e1[i];   // one entry in the ring: _get_delay_obs returns it (minitaur.py:345-346)
  WSYNC();
  PT(29);
  if constexpr (SENS) sensors_push_noisy(S, lane, true, SN, c.seed, ep, 0u);
  else sensors_push(S, lane, true);
  const float e1_keep[2] = {e1[lane], e1[lane < 3 ? 16 + lane : lane]};   // ring entry #1: words lane and (lanes 0..2) 16 + lane
  PT(18);
  // 4b. randomiser (controllable_env_randomizer_from_config.py:92-122), sorted-name draw order:
  //    inertia 2 | joint friction 8 | latency 1 | lateral friction 1 | mass 2 | motor strength 12
  if constexpr (RAND) {
    // Table-driven (orr_set_randomizer): value = fmaf(u, hi - lo, lo); a disabled parameter leaves its words alone; the reference's
    // application order (sorted by name) decides where two parameters write the same word.  ONE lane owns each word and picks the last
    // enabled writer's value in registers - no order of LDS stores by different lanes to lean on: lanes 0..11 their STRENGTH word
    // (single leg weaken over motor strength over leg weaken over global motor strength), lanes 0..13 the word of draw `lane` as in the
    // loop below (lane 12: mass over base mass).  u comes from the draws or, suspended, from the row
    if (c.flags & ORR_FLAG_RANDOMIZER) {
      const bool susp = RR->suspend;
      const float u_a = susp ? row_a : draws[lane], u_ms = susp ? row_ms : draws[lane < 12 ? 14 + lane : 0];
      const float u_g = susp ? row_x[1] : xb[1], u_lw = susp ? row_x[3] : xb[3], u_s = susp ? row_x[4] : xb[4], u_bm = susp ? row_x[0] : xb[0];
      // the weakened leg: (m * 4) >> 24, m = the draw's 24-bit integer (as the clip draw)
      const float f_leg = susp ? row_x[2] : (float)((((uint32_t)(xb[2] * 16777216.0f)) * 4u) >> 24);
      // the new episode's row, words lane and 16 + lane (the caller stores it; not while suspended)
      RR->a = u_a;
      RR->b = lane < 10 ? draws[16 + lane]
                        : (lane == 10 ? u_bm : (lane == 11 ? u_g : (lane == 12 ? f_leg : (lane == 13 ? u_lw : (lane == 14 ? u_s : 0.0f)))));
      const float v_a = fmaf(u_a, rn_hi - rn_lo, rn_lo);
      const float v_ms = fmaf(u_ms, rn_hi_u[0] - rn_lo_u[0], rn_lo_u[0]), v_g = fmaf(u_g, rn_hi_u[1] - rn_lo_u[1], rn_lo_u[1]);
      const float v_lw = fmaf(u_lw, rn_hi_u[2] - rn_lo_u[2], rn_lo_u[2]), v_s = fmaf(u_s, rn_hi_u[3] - rn_lo_u[3], rn_lo_u[3]);
      const float v_bm = fmaf(u_bm, rn_hi_u[4] - rn_lo_u[4], rn_lo_u[4]);
      if (lane < 12) {
        float v = v_g;
        if (rn_en_u[2]) v = (float)(lane / 3) == f_leg ? v_lw : 1.0f;
        if (rn_en_u[0]) v = v_ms;
        if (rn_en_u[3]) v = lane < 3 ? v_s : 1.0f;
        if (rn_en_u[0] | rn_en_u[1] | rn_en_u[2] | rn_en_u[3]) S.s[O(STRENGTH) + lane] = v;
      }
      if (lane < 2) { if (rn_en) S.s[O(INERTIA_RATIO) + lane] = v_a; }
      else if (lane < 10) { if (rn_en && (lane & 1) == 0) S.s[O(KNEE_FRICTION) + ((lane - 2) >> 1)] = v_a; }
      else if (lane == 10) { if (rn_en) S.s[O(LATENCY)] = v_a; }
      else if (lane == 11) { if (rn_en) S.s[O(FOOT_MU)] = v_a; }
      else if (lane == 12) { if (rn_en | rn_en_u[4]) S.s[O(MASS_RATIO)] = rn_en ? v_a : v_bm; }
      else if (lane == 13) { if (rn_en) S.s[O(MASS_RATIO) + 1] = v_a; }
      WSYNC();
    }
  } else if (c.flags & ORR_FLAG_RANDOMIZER) {
    for (int i = lane; i < 26; i += kLanes) {
      const float u = draws[i];
      if (i < 2) S.s[O(INERTIA_RATIO) + i] = 0.5f + u * 1.0f;
      else if (i < 10) { if (((i - 2) & 1) == 0) S.s[O(KNEE_FRICTION) + ((i - 2) >> 1)] = u * 0.05f; }
      else if (i == 10) S.s[O(LATENCY)] = u * 0.04f;
      else if (i == 11) S.s[O(FOOT_MU)] = 0.5f + u * 0.75f;
      else if (i < 14) S.s[O(MASS_RATIO) + i - 12] = 0.8f + u * 0.4f;
      else S.s[O(STRENGTH) + i - 14] = 0.8f + u * 0.4f;
    }
    WSYNC();   // the new mass / inertia ratios take effect in the next launch's load_leg_const (no staged mass table any more)
  }
  PT(25);
  // 5b. the reference poses of the start time: the wait for the frames, with no store or atomic of this wave in front of it
  sample_poses_finish(P, S, lane, tl, true, PL, 26);
  PT(21);
  if (lane == 0) {
    // origin offset: position first (with identity rotation), then rotation; position is NOT recomputed
    // afterwards (imitation_task.py:712-723)
    S.s[O(ORIGIN_POS)] = S.s[O(POS)] - S.ph.end.pose[0][0];
    S.s[O(ORIGIN_POS) + 1] = S.s[O(POS) + 1] - S.ph.end.pose[0][1];
    S.s[O(ORIGIN_POS) + 2] = 0.0f;
    const float dh = qheading(&S.s[O(QUAT)]) - qheading(&S.ph.end.pose[0][3]);
    q_about_z(dh, &S.s[O(ORIGIN_ROT)]);
    S.s[O(PREV_PHASE)] = clip_phase(clip, t);
  }
  if constexpr (CLIPS) *clip_change = clip_change_time(t, sw_min, sw_max, u_change);   // the record's CLIP_CHANGE_TIME: store_reset_extras
  WSYNC();
  apply_origin(S, lane, 5);
  for (int i = lane; i < 19; i += kLanes) S.s[O(REF_POSE) + i] = S.ph.end.pose[0][i];
  if (lane == 0) {
    float v[3];
    qrot(&S.ph.end.vel[0], &S.s[O(ORIGIN_ROT)], v); S.ph.end.vel[0] = v[0]; S.ph.end.vel[1] = v[1]; S.ph.end.vel[2] = v[2];
    qrot(&S.ph.end.vel[3], &S.s[O(ORIGIN_ROT)], v); S.ph.end.vel[3] = v[0]; S.ph.end.vel[4] = v[1]; S.ph.end.vel[5] = v[2];
  }
  WSYNC();
  for (int i = lane; i < 18; i += kLanes) S.s[O(REF_VEL) + i] = S.ph.end.vel[i];
  // 6. _sync_sim_model / _set_state (:778-829): teleport the sim robot onto the reference
  if (lane < 3) { S.s[O(POS) + lane] = S.ph.end.pose[0][lane]; S.s[O(LINVEL) + lane] = S.ph.end.vel[lane]; S.s[O(ANGVEL) + lane] = S.ph.end.vel[3 + lane]; }
  if (lane < 4) S.s[O(QUAT) + lane] = S.ph.end.pose[0][3 + lane];
  if (lane < 12) { S.s[O(Q) + lane] = S.ph.end.pose[0][7 + lane]; S.s[O(QD) + lane] = S.ph.end.vel[6 + lane]; }
  if constexpr (NOISE) {
    // _apply_state_perturb (:1199-1243) on what was just written, by the lanes that wrote it (same lane, same word, in order); REF_POSE,
    // REF_VEL, the origin and PREV_PHASE above keep the unperturbed state.  One fused multiply-add per word: reference + std z, rounded once
    if (nz[0] < n_prob) {
      const float* z = nz + 4;
      if (lane < 2) { S.s[O(POS) + lane] = fmaf(n_pos, z[lane], S.ph.end.pose[0][lane]); S.s[O(LINVEL) + lane] = fmaf(n_vel, z[15 + lane], S.ph.end.vel[lane]); }
      if (lane < 3) S.s[O(ANGVEL) + lane] = fmaf(n_ang, z[17 + lane], S.ph.end.vel[3 + lane]);
      if (lane < 12) { S.s[O(Q) + lane] = fmaf(n_jp, z[3 + lane], S.ph.end.pose[0][7 + lane]); S.s[O(QD) + lane] = fmaf(n_jv, z[20 + lane], S.ph.end.vel[6 + lane]); }
      // quaternion_about_axis(std z2, a) (x) reference rotation, a_i = -1 + 2 U(i) normalised, not renormalised afterwards.  A zero axis
      // (squared norm below 1e-30, probability 2^-72: the reference divides by zero there) is no rotation.  Every lane evaluates it, lanes 0..3 store
      const float a0 = fmaf(2.0f, nz[1], -1.0f), a1 = fmaf(2.0f, nz[2], -1.0f), a2 = fmaf(2.0f, nz[3], -1.0f);
      const float n2 = a0 * a0 + a1 * a1 + a2 * a2;
      float sh, ch;
      joint_sincos(0.5f * (n_rot * z[2]), &sh, &ch);
      const float ax = n2 < 1e-30f ? 0.0f : sh * rsq(n2);
      const float dq[4] = {a0 * ax, a1 * ax, a2 * ax, n2 < 1e-30f ? 1.0f : ch};
      float qp[4];
      qmul(dq, &S.ph.end.pose[0][3], qp);
      if (lane < 4) S.s[O(QUAT) + lane] = pick4(lane, qp[0], qp[1], qp[2], qp[3]);
    }
  }
  WSYNC();
  PT(22);
  float* e2 = reset_entry2(S);
  receive_obs(S, lane, RC, e2);  // ring entry #2 (imitation_task.py:792)
  {
    // control observation with two entries in the ring (Minitaur._get_delay_obs, minitaur.py:336-357): latency <= 0 -> newest;
    // int(latency / dt) + 1 >= 2 -> the OLDEST entry (#1, the default pose: SURVEY 8a quirk 3); else blend newest / #1
    const float lat = S.s[O(LATENCY)], dt = c.sim_dt;
    const int n = (int)(lat / dt);
    const float al = (lat - n * dt) / dt;
    WSYNC();
    for (int i = lane; i < 19; i += kLanes) {
      const float newest = e2[i], oldest = i < 16 ? e1_keep[0] : e1_keep[1];
      S.co[i] = lat <= 0.0f ? newest : (n + 1 >= 2 ? oldest : (1.0f - al) * newest + al * oldest);
    }
    WSYNC();
  }
  if (lane == 0) seti(S, O(MAX_EP_STEPS), time_limit(c, total_step_count));
  PT(23);
  return ep;
}

// The record's words that a reset writes outside the state head: ring slots 0 and 1 (entries #1 and #2 of reset_robot_state, still in
// LDS) and, CLIPS, the first clip change of the new episode.  Called at the end of the kernel, with the record's other stores
template <bool CLIPS = false>
__device__ __forceinline__ void store_reset_extras(float* rec, Shared& S, int lane, bool valid, float clip_change) {
  store_ring_entry(rec, lane, valid, 0, reset_entry1(S));
  store_ring_entry(rec, lane, valid, 1, reset_entry2(S));
  if constexpr (CLIPS) { if (valid && lane == 0) rec[O(CLIP_CHANGE_TIME)] = clip_change; }
}

// RAND: the params buffer of the handle (orr_bind_randomizer_params), the same in every lane: `robot`'s row, and whether resets apply
// it instead of drawing.  A padding lane group shadows robot 0's row and never stores
__device__ __forceinline__ RandRow load_rand_row(const KParams& P, int robot) {
  const unsigned long long p = *(const unsigned long long __attribute__((address_space(1)))*)&P.tab->rand_params;
  const int s = *(const int __attribute__((address_space(1)))*)&P.tab->rand_suspend;
  const unsigned int plo = __builtin_amdgcn_readfirstlane((unsigned int)p), phi = __builtin_amdgcn_readfirstlane((unsigned int)(p >> 32));
  float* const base = reinterpret_cast<float*>(((unsigned long long)phi << 32) | plo);
  RandRow RR;
  RR.row = base ? base + (size_t)robot * ORR_RAND_ROW : nullptr;
  RR.suspend = base != nullptr && __builtin_amdgcn_readfirstlane(s) != 0;
  return RR;
}
// The new episode's row, words lane and 16 + lane: with the record's stores, behind every load.  Not while suspended (the caller owns
// the rows), not without ORR_FLAG_RANDOMIZER (nothing was drawn)
__device__ __forceinline__ void store_rand_row(const KParams& P, const RandRow& RR, int lane, bool valid) {
  if (valid && RR.row && !RR.suspend && (P.cfg.flags & ORR_FLAG_RANDOMIZER)) {
    float __attribute__((address_space(1)))* const r = (float __attribute__((address_space(1)))*)RR.row;
    r[lane] = RR.a; r[16 + lane] = RR.b;
  }
}

// Philox blocks of the pushes (orr_set_push): A = 0x50000000 + 2 s, B = A + 1, s = the env-step counter before the step
constexpr uint32_t kPushBlock = 0x50000000u;
// PUSH: the outputs buffer of the handle (NULL = not bound) and whether its auto-reset is the table-driven one, the same in every lane
__device__ __forceinline__ void load_push_end(const KParams& P, float** out, bool* table) {
  const unsigned long long p = *(const unsigned long long __attribute__((address_space(1)))*)&P.tab->push_out;
  const int t = *(const int __attribute__((address_space(1)))*)&P.tab->push_table;
  const unsigned int plo = __builtin_amdgcn_readfirstlane((unsigned int)p), phi = __builtin_amdgcn_readfirstlane((unsigned int)(p >> 32));
  *out = reinterpret_cast<float*>(((unsigned long long)phi << 32) | plo);
  *table = __builtin_amdgcn_readfirstlane(t) != 0;
}
// PUSH: the handle's push settings and outputs buffer, each the same in every lane (scalar registers from here on)
__device__ __forceinline__ PushSet load_push(const KParams& P) {
  typedef const float __attribute__((address_space(1)))* gfp;
  const gfp pp = (gfp)&P.tab->push.prob;
  static_assert(offsetof(orr_push, lin_lo) == 4 && offsetof(orr_push, lin_hi) == 8 && offsetof(orr_push, lin_z) == 12 && offsetof(orr_push, ang) == 16 &&
                offsetof(orr_push, grace_steps) == 20, "words 0..5");
  PushSet PS;
  load_push_end(P, &PS.out, &PS.table);
  PS.prob = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pp[0])));
  PS.lin_lo = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pp[1])));
  PS.span = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pp[2]))) - PS.lin_lo;
  PS.lin_z = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pp[3])));
  PS.ang = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pp[4])));
  PS.grace = __builtin_amdgcn_readfirstlane(__float_as_int(pp[5]));
  return PS;
}

// 7. observation = sensor histories + target observation (quadruped_gym_env.py:100-102; wrapper_env.py:101-105, 109-125), for the
// step that just ended and for a reset alike: `episode` / `noise_i` are the robot's own (a reset: the new episode, 0)
template <bool NOISE = false, bool SENS = false>
__device__ static void build_obs(const KParams& P, const float* rec, Shared& S, int lane, float* obs, uint32_t episode, uint32_t noise_i,
                                 const SensorNoise& SN = SensorNoise{}) {
  if (lane < 12) obs[lane] = S.s[O(IMU_HIST) + lane];
  for (int i = lane; i < 36; i += kLanes) { obs[12 + i] = S.s[O(LASTACT_HIST) + i]; obs[48 + i] = S.s[O(MOTORANG_HIST) + i]; }
  target_obs<NOISE, SENS>(P, rec, S, lane, obs + ORR_PROPRIO_DIM, episode, noise_i, SN);
}
