// orr_kernels_push.hip -- eleventh translation unit of the env kernels: ONLY the push instantiation (orr_set_push,
// orr_bind_push_outputs) - the env step orr_step_kernel<kModePush | kModeRandomizer | kModeSensor | kModeActuator | kModeContacts |
// kModeTerms | 0, 1, false, true, true> - and its launcher, compiled with the main unit's flags.  A superset of the randomiser variant:
// unbound outputs are skipped, absent limits pass the torques, a deviation of 0 passes the reading, a robot that is not kicked keeps its
// velocities bit for bit.  No reset and no parity replay of its own: a handle with pushes launches the randomiser unit's.  Its own unit
// for the same reason as orr_kernels_anchor.hip.
#include "orr_env_kernels.h"
template orr::StepLaunch orr::launch_step<orr::kModePush | orr::kModeRandomizer | orr::kModeSensor | orr::kModeActuator | orr::kModeContacts | orr::kModeTerms | 0, 1, false, true, true>;
