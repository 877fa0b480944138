// orr_kernels_terms.hip -- sixth translation unit of the env kernels: ONLY the reward-terms instantiations of the step kernel (the env
// step orr_step_kernel<kModeTerms | 0, 1, false, true, true> and its parity replay <kModeTerms | 2, ...>: lanes 0..4 of a robot also store the
// five unweighted terms of the step's reward, their running sums over the episode and, when the episode ends, the sums' row of the
// episode log, orr_bind_reward_terms) and their launchers, compiled with the main unit's flags.  TERMS comes with CLIPS and NOISE only: the
// noise code is a superset of the clip-set and the default ones (all noise zero and no clip set = the default behaviour), so one
// variant serves the terms with and without either.  Resets of such a handle run the noise unit's reset kernel: the sums restart
// inside the step.  Its own unit for the same reason as orr_kernels_anchor.hip.
#include "orr_env_kernels.h"
template orr::StepLaunch orr::launch_step<orr::kModeTerms | 0, 1, false, true, true>;
template orr::StepLaunch orr::launch_step<orr::kModeTerms | 2, 1, false, true, true>;
