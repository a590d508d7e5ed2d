// geo4d_amd/csrc/gemm_v3_bf16x3_up2.hip — the third generation's sub-pixel Upsample kernels (geo4d_conv_gemm_up2: tile hints 71, 72)
// for element type bf16x3_t (a translation unit of their own: parallel build).
#include "gemm_kernel_v3.h"

namespace geo4d_gemm {
template int launch_v3_up2<bf16x3_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
}  // namespace geo4d_gemm
