// ORACLE — test infrastructure only.  Stand-in for the CUDA half header.
#pragma once
#include <hip/hip_fp16.h>
