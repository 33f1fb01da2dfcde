// Indicator kriging, 3-D: the compile-time kinds of the median form of ik_local_kernel (ik_kernel.h).
#include "ik_kernel.h"

namespace gss {

int32_t ik_local_launch_3d(int kind, const IkLaunch& a) { return ik_local_launch_kinds<3>(kind, a); }

}  // namespace gss
