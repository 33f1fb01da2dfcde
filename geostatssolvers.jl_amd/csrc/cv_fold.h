// What the cross-validation entry points share (krig_cv.hip, idw_lwr.hip): the check of the caller's fold ids and the
// exclusion ball in the units of the search key.
#pragma once

#include "gss_internal.h"

#include <vector>

namespace gss {

// The fold ids of n samples where the host can read them (own->data() after a copy of device memory, else `fold`
// itself), none of them negative: they are checked before any kernel indexes or compares by them.
inline int32_t fold_ids_host(const char* who, const int32_t* fold, int64_t n, int32_t mem, hipStream_t s,
                             std::vector<int32_t>* own) {
  if (mem != GSS_MEM_HOST) {
    own->resize((size_t)n);
    GSS_HIP(hipMemcpyAsync(own->data(), fold, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    GSS_HIP(hipStreamSynchronize(s));
    fold = own->data();
  }
  for (int64_t i = 0; i < n; ++i)
    GSS_REQUIRE(fold[i] >= 0, "%s: fold id %d of sample %lld is negative", who, fold[i], (long long)i);
  return GSS_OK;
}

// the exclusion ball in the search key: squared (and scaled like the ball) for the Euclidean family, else as it is
inline double exclusion_key(double exclude_radius, int metric) {
  if (exclude_radius < 0.0) return -1.0;
  return metric == GSS_METRIC_EUCLIDEAN ? exclude_radius * exclude_radius : exclude_radius;
}

}  // namespace gss
