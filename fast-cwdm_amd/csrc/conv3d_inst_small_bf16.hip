// Explicit instantiation: small-grid conv kernels, bf16.
#include "conv3d_kernels.hpp"
namespace cwdm {
CWDM_SMALL_INSTANCES(template, bf16_t)
}  // namespace cwdm
