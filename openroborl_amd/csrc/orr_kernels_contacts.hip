// orr_kernels_contacts.hip -- seventh translation unit of the env kernels: ONLY the contact-output instantiations of the step kernel (the
// env step orr_step_kernel<kModeContacts | 0, 1, false, true, true>, the same with the reward terms <kModeContacts | kModeTerms | 0, ...>, so
// that both bindings can be active at once, and the debug physics <kModeContacts | 1, 1, false, false>: lanes 0..11 of a robot also sum the
// contact impulses of every sub-step, orr_bind_contact_outputs) and their launchers, compiled with the main unit's flags.  The env step
// comes with CLIPS and NOISE only, a superset as in orr_kernels_terms.hip.  Resets of such a handle run the noise unit's reset kernel:
// the episode totals restart inside the step.  No parity replay: it has no impulses.  Its own unit for the same reason as
// orr_kernels_anchor.hip.
#include "orr_env_kernels.h"
template orr::StepLaunch orr::launch_step<orr::kModeContacts | 0, 1, false, true, true>;
template orr::StepLaunch orr::launch_step<orr::kModeContacts | orr::kModeTerms | 0, 1, false, true, true>;
template orr::StepLaunch orr::launch_step<orr::kModeContacts | 1, 1, false, false>;
