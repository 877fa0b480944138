// orr_kernels_noise.hip -- fifth translation unit of the env kernels: ONLY the task-noise instantiations of the step kernel and the reset
// kernel (orr_step_kernel<0, 1, false, true, true>, orr_reset_kernel<true, true>: a reset places the robot on a Gaussian-perturbed copy of
// the reference state with probability perturb_init_state_prob, and every target observation is expressed in a noisy heading,
// orr_set_task_noise), the step's parity replay (orr_step_kernel<2, 1, false, true, true>) and their launchers, compiled with the main
// unit's flags.  NOISE comes with CLIPS only: the clip-set code is a superset of the default one (a robot type without a clip set keeps
// its CLIP_ID, a type without a switch interval never switches), so one variant serves noise with and without clip sets.  Its own unit
// for the same reason as orr_kernels_anchor.hip.
#include "orr_env_kernels.h"
template orr::StepLaunch orr::launch_step<0, 1, false, true, true>;
template orr::ResetLaunch orr::launch_reset<true, true>;
template orr::StepLaunch orr::launch_step<2, 1, false, true, true>;
