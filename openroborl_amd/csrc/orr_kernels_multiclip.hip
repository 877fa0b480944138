// orr_kernels_multiclip.hip -- fourth translation unit of the env kernels: ONLY the clip-set instantiations of the step kernel and the
// reset kernel (orr_step_kernel<0, 1, false, true>, orr_reset_kernel<true>: every reset draws the episode's clip from the robot type's
// clip set, orr_set_clip_set, by the type's thresholds in the device table - uniform, orr_set_clip_weights' or the ones
// orr_clip_curriculum_update wrote; a robot whose clip switch time has come switches clips mid-episode, orr_set_clip_switch), the step's parity
// replay (orr_step_kernel<2, 1, false, true>, run while some type has a switch interval) and their launchers, compiled with the main
// unit's flags.  Its own unit for the same reason as orr_kernels_anchor.hip.
#include "orr_env_kernels.h"
template orr::StepLaunch orr::launch_step<0, 1, false, true>;
template orr::ResetLaunch orr::launch_reset<true>;
template orr::StepLaunch orr::launch_step<2, 1, false, true>;
