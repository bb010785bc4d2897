// Stand-in for the CUDA toolkit's cuda_runtime.h: TEST INFRASTRUCTURE, used only to let the
// reference's shared per-element headers compile for the host (oracle/Makefile, target ref).
// Declarations only -- this file holds no arithmetic; nothing computed by ref_pin_stages comes
// from here.  (HIP's own runtime header is not used: its atomicMin(float*) collides with the
// one the reference declares itself.)
#pragma once
#include <cstddef>
#include <limits>

#define __host__ __attribute__((host))
#define __device__ __attribute__((device))
#define __global__ __attribute__((global))
#define __shared__ __attribute__((shared))
#define __constant__ __attribute__((constant))

struct dim3 {
    unsigned x, y, z;
    __host__ __device__ dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct uint3 { unsigned x, y, z; };
extern const __device__ uint3 threadIdx, blockIdx;
extern const __device__ dim3 blockDim, gridDim;

typedef int cudaError;
typedef cudaError cudaError_t;
static const cudaError cudaSuccess = 0;
const char* cudaGetErrorString(cudaError err);

// what clang lowers a <<<grid, block>>> launch to in HIP mode
extern "C" int __hipPushCallConfiguration(dim3 gridSize, dim3 blockSize, size_t sharedMem = 0, void* stream = 0);

__device__ int atomicAdd(int* address, int val);
__device__ unsigned atomicAdd(unsigned* address, unsigned val);
__device__ float atomicAdd(float* address, float val);
__device__ int atomicCAS(int* address, int compare, int val);
__device__ int __float_as_int(float x);
__device__ float __int_as_float(int x);
__device__ void __syncthreads();
