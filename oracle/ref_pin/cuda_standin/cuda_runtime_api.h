// Stand-in for the CUDA toolkit header of this name: declarations only, no arithmetic;
// everything is in cuda_runtime.h beside it.
#pragma once
#include "cuda_runtime.h"
