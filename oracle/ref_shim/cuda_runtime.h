// ORACLE — test infrastructure only.  Stand-in for the CUDA runtime header.
#pragma once
#include <hip/hip_runtime.h>
