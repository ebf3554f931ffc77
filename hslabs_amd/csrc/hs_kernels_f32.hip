// hs_kernels_f32.hip -- the fp32 unit of the step kernels (BASELINE configs[2]: spider, 16384 rollouts x
// horizon 32, fp32): the same headers with `real` = float and the launcher table hs::kernels_f32. All
// arithmetic, LDS and outputs in float; topology and gait parameters are converted on load.
#define HS_REAL float
#define HS_REAL_IS_FLOAT 1
#include "hs_rollout_kernel.h"
#include "hs_limb.h"

namespace hs {

#ifndef __HIP_DEVICE_COMPILE__  // host only: the device pass would emit a constant-initialised const object too
extern const kernels kernels_f32 = {general_workspace_bytes, launch_rollouts,     launch_fused,
                                    launch_limb,             launch_fused_reduce, limb_deferred};
#endif

}  // namespace hs
