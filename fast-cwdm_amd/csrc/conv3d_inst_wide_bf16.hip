// Explicit instantiation: wide-grid conv kernels, bf16.
#include "conv3d_kernels.hpp"
namespace cwdm {
CWDM_WIDE_INSTANCES(template, bf16_t)
}  // namespace cwdm
