// Explicit instantiation: small-grid conv kernels, f32.
#include "conv3d_kernels.hpp"
namespace cwdm {
CWDM_SMALL_INSTANCES(template, float)
}  // namespace cwdm
