// orr_variants.h -- which instantiation of the env kernels an entry point of the C-ABI launches: one pure rule.
//
// Host only, plain C++17, no HIP header: orr_kernels.hip asks it for every launch, and tests/host_probe/orr_variant_probe.cpp
// walks it without a GPU.  The rule knows no handle and no launcher: orr_kernels.hip reads the handle's switches into Features
// (features_of) and maps the Variant it gets onto a launcher, one table per entry point.
#pragma once
#include <stddef.h>
#include <stdio.h>

namespace orr {

enum Variant { kRefused = -1, kDefault, kTwoWave, kAnchor, kClips, kNoise, kTerms, kContacts, kContactsTerms, kActuator, kSensor, kRandomizer, kPush, kNumVariants };
constexpr const char* kVariantNames[] = {"kDefault", "kTwoWave", "kAnchor", "kClips", "kNoise", "kTerms", "kContacts", "kContactsTerms",
                                         "kActuator", "kSensor", "kRandomizer", "kPush"};
static_assert(sizeof(kVariantNames) / sizeof(kVariantNames[0]) == kNumVariants, "one name per variant");

enum Entry { kEntryStep, kEntryReset, kEntryDebugPhysics, kEntryReplayStep, kEntryReplayReset, kNumEntries };
constexpr const char* kEntryNames[] = {"orr_step", "orr_reset", "orr_debug_physics", "orr_debug_replay_step", "orr_debug_replay_reset"};
static_assert(sizeof(kEntryNames) / sizeof(kEntryNames[0]) == kNumEntries, "one name per entry point");

// What is switched on, as the entry point sees it (`clips`: a clip set of more than one clip for step and reset, a finite clip switch
// interval for the parity replays; `two_wave`: more waves than SIMDs, or ORR_STEP_WAVES_PER_EU=2)
struct Features { bool anchors, clips, noise, terms, contacts, actuator, sensor, randomizer, push, two_wave; };

// `conflict`: with kRefused, what the friction anchors cannot be combined with (format_anchor_conflict); else null
struct Choice { Variant variant; const char* conflict; };

// Every feature's variants are supersets of the variants of the features below it, so the first feature that is on decides.  No
// feature has an anchor instantiation: with an anchor model (set after the feature was switched on - the setters refuse the other
// order) the call is refused, whether or not the entry point has a variant for the feature.  An entry point without one goes on down
// the list and launches what it launches without the feature.
inline Choice choose_variant(const Features& f, Entry e) {
  constexpr const char* contacts = "contact outputs (orr_bind_contact_outputs)";
  if (e == kEntryDebugPhysics) {   // fixed torques, no task: contact sums or friction anchors are all it can differ by, and it has no two-wave form
    if (f.contacts) return f.anchors ? Choice{kRefused, contacts} : Choice{kContacts, nullptr};
    return {f.anchors ? kAnchor : kDefault, nullptr};
  }
  const bool step = e == kEntryStep, replay = e == kEntryReplayStep || e == kEntryReplayReset;
  const struct { bool on, here; Variant variant; const char* phrase; } rows[] = {
      {f.push, step, kPush, "pushes (orr_set_push, orr_bind_push_outputs)"},
      {f.randomizer, true, kRandomizer, "the randomiser (orr_set_randomizer, orr_bind_randomizer_params)"},
      {f.sensor, true, kSensor, "sensor noise (orr_set_sensor_noise)"},
      {f.actuator, true, kActuator, "torque limits / actuator outputs (orr_set_torque_limits, orr_bind_actuator_outputs)"},
      // the parity replays have no impulses: they do not look at the binding at all and leave contact_out alone
      {f.contacts && !replay, true, step && f.terms ? kContactsTerms : kContacts, contacts},
      {f.terms, true, kTerms, "reward terms (orr_bind_reward_terms)"},
      {f.noise, true, kNoise, "task noise (orr_set_task_noise)"},
      {f.clips, true, kClips, "a clip set of more than one clip"},
  };
  for (const auto& r : rows) {
    if (!r.on) continue;
    if (f.anchors) return {kRefused, r.phrase};
    if (r.here) return {r.variant, nullptr};
  }
  if (f.anchors) return {kAnchor, nullptr};
  return {f.two_wave ? kTwoWave : kDefault, nullptr};
}

// the message of a refusal: it starts with the entry point's name
inline int format_anchor_conflict(char* out, size_t size, Entry e, const char* conflict) {
  return snprintf(out, size, "%s: friction anchors (orr_model::friction_anchor) and %s cannot be combined", kEntryNames[e], conflict);
}

}  // namespace orr
