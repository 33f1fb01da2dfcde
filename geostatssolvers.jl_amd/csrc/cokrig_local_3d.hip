// Moving-neighbourhood cokriging, 3-D: the compile-time kinds of cokrig_local_kernel and cokrig_cv_kernel
// (cokrig_local_kernel.h).
#include "cokrig_local_kernel.h"

namespace gss {

int32_t cokrig_local_launch_3d(int kind, const CoLocalLaunch& a) { return cokrig_local_launch_kinds<3>(kind, a); }
int32_t cokrig_cv_launch_3d(int kind, const CoLocalLaunch& a) { return cokrig_local_launch_kinds<3, true>(kind, a); }

}  // namespace gss
