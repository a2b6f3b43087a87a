// the elastic-net trial kernels (zf_trial_enet_kernel): gradient vector in HBM, single trials, with and without history
#include "zf_trial_launch.h"

void zf_launch_enet(const zf_trial_sel& v, bool hist, int grid, hipStream_t st, const zf_step_args& a, double l2) {
#define CALL(N, B)                                                                                                          \
    do {                                                                                                                    \
        if (hist) hipLaunchKernelGGL((zf_trial_enet_kernel<N, B, true>), dim3(grid), dim3(ZF_BLOCK), 0, st, a, l2);         \
        else hipLaunchKernelGGL((zf_trial_enet_kernel<N, B, false>), dim3(grid), dim3(ZF_BLOCK), 0, st, a, l2);             \
    } while (0)
    ZF_SEL_NB(v, CALL);
#undef CALL
}
