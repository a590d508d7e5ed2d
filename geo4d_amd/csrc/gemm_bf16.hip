// geo4d_amd/csrc/gemm_bf16.hip — conv_gemm kernels for element type bf16_t (one translation unit per type: parallel build).
#include "gemm_kernel.h"

namespace geo4d_gemm {
template int launch_typed<bf16_t>(const geo4d_conv_gemm_t&, const Plan&, hipStream_t);
}  // namespace geo4d_gemm
