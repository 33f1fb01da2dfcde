// Indicator kriging, 2-D: the compile-time kinds of the median form of ik_local_kernel (ik_kernel.h).
#include "ik_kernel.h"

namespace gss {

int32_t ik_local_launch_2d(int kind, const IkLaunch& a) { return ik_local_launch_kinds<2>(kind, a); }

}  // namespace gss
