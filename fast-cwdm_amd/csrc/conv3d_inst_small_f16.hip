// Explicit instantiation: small-grid conv kernels, fp16.
#include "conv3d_kernels.hpp"
namespace cwdm {
CWDM_SMALL_INSTANCES(template, f16_t)
}  // namespace cwdm
