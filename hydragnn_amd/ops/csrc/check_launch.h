// Launch check shared by every kernel family: a bad configuration
// (grid, block, dynamic LDS) is reported at the launch, by name, and
// not at some later synchronisation.
#pragma once

#include <torch/extension.h>
#include <hip/hip_runtime.h>

inline void check_launch(const char* what) {
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, what, " launch failed: ",
              hipGetErrorString(err));
}
