// orr_kernels_multiclip.hip -- fourth translation unit of the env kernels: ONLY the clip-set instantiations of the step kernel and the reset
// kernel (orr_step_kernel<0, 1, false, true>, orr_reset_kernel<true>: every reset draws the episode's clip from the robot type's clip set,
// orr_set_clip_set; a robot whose clip switch time has come switches clips mid-episode, orr_set_clip_switch), their parity replays
// (orr_step_kernel<2, 1, false, true>, run while some type has a switch interval) and their launchers, compiled with the main unit's flags.  Its own unit so that the default kernels' code generation does
// not depend on this feature being compiled next to them (the precedent of orr_kernels_anchor.hip; see launch_step_multiclip).
#define ORR_TU_MULTICLIP 1
#include "orr_kernels.hip"
