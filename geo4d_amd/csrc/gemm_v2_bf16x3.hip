// geo4d_amd/csrc/gemm_v2_bf16x3.hip — second-generation conv_gemm kernels (tile hints 22..28) for element type bf16x3_t
// (one translation unit per type: parallel build).
#include "gemm_kernel_v2.h"

namespace geo4d_gemm {
template int launch_v2_typed<bf16x3_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
}  // namespace geo4d_gemm
