// geo4d_amd/csrc/gemm_v2_bf16x3_up2.hip — the second generation's sub-pixel Upsample kernels (geo4d_conv_gemm_up2: tile hints 22, 23, 25)
// for element type bf16x3_t (a translation unit of their own: parallel build).
#include "gemm_kernel_v2.h"

namespace geo4d_gemm {
template int launch_v2_up2<bf16x3_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
}  // namespace geo4d_gemm
