// The quaternion cameras' instantiations of the gradient-only evaluator (line_search_gradient.h; LaunchLsGradient of
// kernels_line_search.hip calls in here, and runs the two finishing kernels afterwards).  A translation unit of their own, as
// kernels_quaternion.hip is for bal_evaluate.h.
#include <hip/hip_runtime.h>

#include "device.h"
#include "line_search_gradient.h"

namespace chip {

namespace {

template <int CM>
hipError_t launch_ls_gradient(const LsGradArgs& A, bool gradient, int gp, int gc, hipStream_t stream) {
  const bool robust = A.loss.type != kLossNone;
  if (!gradient) {
    if (robust) hipLaunchKernelGGL((ls_point_pass_kernel<CM, true, false>), dim3(gp), dim3(kVecBlock), 0, stream, A);
    else hipLaunchKernelGGL((ls_point_pass_kernel<CM, false, false>), dim3(gp), dim3(kVecBlock), 0, stream, A);
    return hipGetLastError();
  }
  if (robust) {
    hipLaunchKernelGGL((ls_point_pass_kernel<CM, true, true>), dim3(gp), dim3(kVecBlock), 0, stream, A);
    hipLaunchKernelGGL((ls_camera_pass_kernel<CM, true>), dim3(gc), dim3(kVecBlock), 0, stream, A);
  } else {
    hipLaunchKernelGGL((ls_point_pass_kernel<CM, false, true>), dim3(gp), dim3(kVecBlock), 0, stream, A);
    hipLaunchKernelGGL((ls_camera_pass_kernel<CM, false>), dim3(gc), dim3(kVecBlock), 0, stream, A);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t LaunchLsGradientQuat(const LsGradArgs& A, bool gradient, int camera_model, int grid_points, int grid_cameras, hipStream_t stream) {
  if (camera_model == kCamQuaternion) return launch_ls_gradient<kCamQuaternion>(A, gradient, grid_points, grid_cameras, stream);
  if (camera_model == kCamQuaternionManifold) return launch_ls_gradient<kCamQuaternionManifold>(A, gradient, grid_points, grid_cameras, stream);
  return hipErrorInvalidValue;
}

}  // namespace chip
