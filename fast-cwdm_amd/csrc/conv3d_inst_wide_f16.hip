// Explicit instantiation: wide-grid conv kernels, fp16.
#include "conv3d_kernels.hpp"
namespace cwdm {
CWDM_WIDE_INSTANCES(template, f16_t)
}  // namespace cwdm
