// ORACLE — test infrastructure only.  Stand-in for the CUDA driver header: the HIP runtime supplies what the reference's kernels use.
#pragma once
#include <hip/hip_runtime.h>
