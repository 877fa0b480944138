// Host probe of the env kernels' variant rule (csrc/orr_variants.h) -- test infrastructure only: plain C++, no device code, loaded
// through ctypes by tests/variant_probe.py.  `mask`: bit i = the i-th member of orr::Features in the order of its declaration.
#include "orr_variants.h"

static orr::Features features_of_mask(unsigned mask) {
  orr::Features f;
  bool* const members[] = {&f.anchors, &f.clips, &f.noise, &f.terms, &f.contacts, &f.actuator, &f.sensor, &f.randomizer, &f.push, &f.two_wave};
  for (unsigned i = 0; i < sizeof(members) / sizeof(members[0]); i++) *members[i] = (mask >> i) & 1u;
  return f;
}

extern "C" {

int orrv_num_variants(void) { return orr::kNumVariants; }
int orrv_num_entries(void) { return orr::kNumEntries; }
const char* orrv_entry_name(int entry) { return orr::kEntryNames[entry]; }
const char* orrv_variant_name(int variant) { return variant == orr::kRefused ? "kRefused" : orr::kVariantNames[variant]; }

int orrv_choose(unsigned mask, int entry) { return orr::choose_variant(features_of_mask(mask), (orr::Entry)entry).variant; }

// the message of a refused call into out[size] (its length is returned); 0 and an empty string where the call is not refused
int orrv_message(unsigned mask, int entry, char* out, int size) {
  const orr::Choice c = orr::choose_variant(features_of_mask(mask), (orr::Entry)entry);
  out[0] = 0;
  return c.variant == orr::kRefused ? orr::format_anchor_conflict(out, (size_t)size, (orr::Entry)entry, c.conflict) : 0;
}

}  // extern "C"
