// the penalty-factor trial kernels (zf_trial_pf_kernel): gradient vector in HBM, single trials, with and without history;
// the factors travel in a.p1
#include "zf_trial_launch.h"

void zf_launch_pf(const zf_trial_sel& v, bool hist, int grid, hipStream_t st, const zf_step_args& a) {
#define CALL(N, B)                                                                                                  \
    do {                                                                                                            \
        if (hist) hipLaunchKernelGGL((zf_trial_pf_kernel<N, B, true>), dim3(grid), dim3(ZF_BLOCK), 0, st, a);       \
        else hipLaunchKernelGGL((zf_trial_pf_kernel<N, B, false>), dim3(grid), dim3(ZF_BLOCK), 0, st, a);           \
    } while (0)
    ZF_SEL_NB(v, CALL);
#undef CALL
}
