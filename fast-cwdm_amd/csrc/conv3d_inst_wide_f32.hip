// Explicit instantiation: wide-grid conv kernels, f32.
#include "conv3d_kernels.hpp"
namespace cwdm {
CWDM_WIDE_INSTANCES(template, float)
}  // namespace cwdm
