// orr_kernels_randomizer.hip -- tenth translation unit of the env kernels: ONLY the randomiser instantiations (orr_set_randomizer,
// orr_bind_randomizer_params: ControllableEnvRandomizerFromConfig) - the env step orr_step_kernel<kModeRandomizer | kModeSensor |
// kModeActuator | kModeContacts | kModeTerms | 0, 1, false, true, true>, the parity replay <kModeRandomizer | kModeSensor | kModeActuator |
// kModeTerms | 2, ...> and the reset orr_randomizer_reset_kernel<true> - and their launchers, compiled with the main unit's flags.  All
// three are supersets of the sensor variants: unbound outputs are skipped, absent limits pass the torques, a deviation of 0 passes the
// reading.  Its own unit for the same reason as orr_kernels_anchor.hip.
#include "orr_env_kernels.h"
template orr::StepLaunch orr::launch_step<orr::kModeRandomizer | orr::kModeSensor | orr::kModeActuator | orr::kModeContacts | orr::kModeTerms | 0, 1, false, true, true>;
template orr::StepLaunch orr::launch_step<orr::kModeRandomizer | orr::kModeSensor | orr::kModeActuator | orr::kModeTerms | 2, 1, false, true, true>;
template orr::ResetLaunch orr::launch_randomizer_reset<true>;
