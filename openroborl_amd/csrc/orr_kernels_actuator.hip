// orr_kernels_actuator.hip -- eighth translation unit of the env kernels: ONLY the actuator instantiations of the step kernel (the env step
// orr_step_kernel<kModeActuator | kModeContacts | kModeTerms | 0, 1, false, true, true> and the parity replay <kModeActuator | kModeTerms | 2,
// ...>: lane = motor clips the sub-step's torque to its motor's limit and keeps sum tau, max |tau|, sum tau^2 and the work over the launch's
// sub-steps, orr_set_torque_limits / orr_bind_actuator_outputs) and their launchers, compiled with the main unit's flags.  Both are supersets:
// they hold the reward-terms code (the env step the contact sums too) and skip that binding's loads and stores where its pointer is
// null, so that two kernels serve every combination of the three bindings.  Resets of such a handle run the noise unit's reset kernel:
// the episode totals restart inside the step.  No debug physics: it takes its torques as given.  Its own unit for the same reason as
// orr_kernels_anchor.hip.
#include "orr_env_kernels.h"
template orr::StepLaunch orr::launch_step<orr::kModeActuator | orr::kModeContacts | orr::kModeTerms | 0, 1, false, true, true>;
template orr::StepLaunch orr::launch_step<orr::kModeActuator | orr::kModeTerms | 2, 1, false, true, true>;
