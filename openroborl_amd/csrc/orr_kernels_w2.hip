// orr_kernels_w2.hip -- second translation unit of the env kernels: ONLY the two-waves-per-SIMD instantiation of the step kernel
// (orr_step_kernel<0, 2>, for batches of more waves than the device has SIMDs) and its launcher, compiled with its OWN flags
// (-Os + iterative-maxocc: at 256 registers this variant spills, and the main unit's iterative-ilp schedule costs it 8 %;
// openroborl_amd/_lib.py: HIPCC_FLAGS_W2).
#define ORR_TU_STEP_W2 1     // orr_physics.h: this unit's choice of constraint-row code
// start parity of the hand-written Gauss-Seidel loops (orr_device.h): with two waves sharing the instruction fetch the other parity wins
// (8192 robots: 0.3310 ms with the one-wave unit's 0x1000, 0.3259 ms with 0; the one-wave unit the other way round: 0.2344 vs 0.2395)
#ifndef ORR_PARITY
#define ORR_PARITY 0x0000
#endif
#include "orr_env_kernels.h"
template orr::StepLaunch orr::launch_step<0, 2, false, false>;
#ifdef ORR_STAGE_DUMP
template orr::StageDumpLaunch orr::launch_stage_dump<false, 2>;     // development aid: this unit's forms of the sub-step's first half
template orr::StageDumpLaunch orr::launch_stage_dump<true, 2>;
#endif
