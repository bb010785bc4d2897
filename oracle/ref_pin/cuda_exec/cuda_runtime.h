// cuda_exec/cuda_runtime.h -- TEST INFRASTRUCTURE.  EXECUTING stand-ins for the CUDA toolkit headers, so
// that the reference's imgproc.cu and proj_icp.cu compile with plain g++ and their __global__ /
// __device__ bodies run on the host (oracle/ref_pin/ref_pin_front.cpp; oracle/Makefile, target ref).
// Separate from cuda_standin/, which stays declaration-only.  No reference text is here.
//
// UNLIKE cuda_standin THIS FILE HOLDS ARITHMETIC: it is DESIGN.md section 3 (the canonical numerics)
// written as code.  What the pin built on it shows is "the reference's text under section 3", not
// CUDA's own arithmetic (fast intrinsics, --prec-div=false, FMA contraction), which stays unpinned:
//   __fmaf_rn(a, b, c)      -> fmaf(a, b, c)
//   __fdividef(x, y)        -> x * (1.0f / y)
//   rsqrt / rsqrtf(x)       -> 1.0f / sqrtf(x)
//   __float2int_rn(x)       -> round to nearest even (nearbyintf in the default rounding mode); NaN -> 0
//   __int_as_float          -> the bits
//   __expf(x)               -> the ORACLE's tfo_exp (linked from tf_oracle.c): the exp is the oracle's, not
//                              the reference's, and is checked on its own in tests/test_oracle.py
//   tex2D, 2-D point filter -> element (floorf(x), floorf(y)), clamped to the image
//   __syncthreads()         -> nothing; __shared__ -> static (the grid is walked serially, one thread
//                              at a time, so code that exchanges data through shared memory cannot run)
//   cudaMalloc*, cudaMemcpy*, cudaFree*, cudaBindTexture2D -> malloc / memcpy / free / a pointer
// Compile with -ffp-contract=off -fno-fast-math -fwrapv.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#define __host__
#define __device__
#define __global__
#define __shared__ static
#define __forceinline__ inline
#define __CUDACC__ 1

// ---- vector types ------------------------------------------------------------------------------------
struct uint3 { unsigned x, y, z; };
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int3 { int x, y, z; };
struct ushort2 { unsigned short x, y; };
struct uchar4 { unsigned char x, y, z, w; };
typedef unsigned short ushort;
typedef unsigned char uchar;
static inline float2 make_float2(float x, float y) { float2 r = { x, y }; return r; }
static inline float3 make_float3(float x, float y, float z) { float3 r = { x, y, z }; return r; }
static inline float4 make_float4(float x, float y, float z, float w) { float4 r = { x, y, z, w }; return r; }
static inline int3 make_int3(int x, int y, int z) { int3 r = { x, y, z }; return r; }
static inline ushort2 make_ushort2(ushort x, ushort y) { ushort2 r = { x, y }; return r; }
static inline uchar4 make_uchar4(uchar x, uchar y, uchar z, uchar w) { uchar4 r = { x, y, z, w }; return r; }

// ---- the serial grid walk ----------------------------------------------------------------------------
// one definition each, in the program that includes this header
extern uint3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;
namespace cuda_exec {
// kernel<<<grid, block>>>(args); is rewritten by the recipe into launch(grid, block, [&]{ kernel(args); });
template<class F> static inline void launch(dim3 g, dim3 b, F f)
{
    gridDim = g; blockDim = b;
    for (unsigned by = 0; by < g.y; ++by) for (unsigned bx = 0; bx < g.x; ++bx)
        for (unsigned ty = 0; ty < b.y; ++ty) for (unsigned tx = 0; tx < b.x; ++tx) {
            blockIdx.x = bx; blockIdx.y = by; blockIdx.z = 0;
            threadIdx.x = tx; threadIdx.y = ty; threadIdx.z = 0;
            f();
        }
}
typedef void* stream_t;
template<class F> static inline void launch(dim3 g, dim3 b, size_t, stream_t, F f) { launch(g, b, f); }
}

// ---- runtime -----------------------------------------------------------------------------------------
typedef int cudaError_t;
typedef int cudaError;
static const int cudaSuccess = 0;
typedef void* cudaStream_t;
enum { cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice, cudaFuncCachePreferL1 };
static inline const char* cudaGetErrorString(int) { return ""; }
static inline int cudaGetLastError() { return 0; }
static inline int cudaDeviceSynchronize() { return 0; }
template<class F> static inline int cudaFuncSetCacheConfig(F, int) { return 0; }
static inline int cudaMalloc(void** p, size_t n) { *p = malloc(n ? n : 1); return 0; }
static inline int cudaFree(void* p) { free(p); return 0; }
static inline int cudaMallocHost(void** p, size_t n) { *p = malloc(n ? n : 1); return 0; }
static inline int cudaFreeHost(void* p) { free(p); return 0; }
// pitched, padded by whole 32 x 8 CTAs of 16-byte elements in both directions and prefilled
static inline int cudaMallocPitch(void** p, size_t* pitch, size_t width_bytes, size_t rows)
{
    *pitch = (width_bytes + 32 * 16 + 255) / 256 * 256;
    *p = malloc(*pitch * (rows + 8));
    if (*p) memset(*p, 0xA5, *pitch * (rows + 8));
    return 0;
}
static inline int cudaMemcpy(void* d, const void* s, size_t n, int) { memcpy(d, s, n); return 0; }
static inline int cudaMemcpyAsync(void* d, const void* s, size_t n, int, cudaStream_t) { memcpy(d, s, n); return 0; }
static inline int cudaMemcpy2D(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, int)
{
    for (size_t y = 0; y < h; ++y) memcpy((char*)d + y * dp, (const char*)s + y * sp, w);
    return 0;
}

// ---- intrinsics: DESIGN.md section 3 -----------------------------------------------------------------
extern "C" float tfo_exp(float x);                                    // oracle/tf_oracle.c
#define __expf(x) tfo_exp(x)                                           // (a macro: glibc's <math.h> declares a function of this name)
static inline int __float2int_rn(float x) { return x == x ? (int)nearbyintf(x) : 0; }
static inline float __fmaf_rn(float a, float b, float c) { return fmaf(a, b, c); }
static inline float __fdividef(float x, float y) { return x * (1.0f / y); }
static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
static inline float rsqrt(float x) { return 1.0f / sqrtf(x); }
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
static inline void __syncthreads() {}
// named by bodies the pin does not run: the render kernels are emitted, so theirs are defined, and stop the program;
// the others (temp_utils.hpp, pack_tsdf) are declared only
// (macros where glibc's <math.h> declares a function of the name; it declares __cosf and __sinf too)
#define __saturatef(x) (abort(), 0.0f)
#define __powf(x, y) (abort(), 0.0f)
unsigned short __float2half_rn(float); float __half2float(unsigned short);
int __popc(int); int __ballot(int); int __all(int);

// unqualified min / max / abs / isnan; max(int, enum) occurs (proj_icp.cu, allocate_buffer)
static inline int max(int a, int b) { return a > b ? a : b; }
static inline int min(int a, int b) { return a < b ? a : b; }
using std::min; using std::max; using std::abs; using std::isnan;

// ---- textures: 2-D, point filtered ---------------------------------------------------------------------
enum cudaTextureReadMode { cudaReadModeElementType };
enum { cudaFilterModePoint };
struct cudaChannelFormatDesc { int unused; };
template<class T> static inline cudaChannelFormatDesc cudaCreateChannelDesc() { return cudaChannelFormatDesc(); }
struct textureReference { int filterMode; const void* data; int cols, rows; size_t step; };
template<class T, int D, cudaTextureReadMode M = cudaReadModeElementType> struct texture : textureReference {};
template<class T, cudaTextureReadMode M>
static inline int cudaBindTexture2D(size_t*, const texture<T, 2, M>& t, const void* p, const cudaChannelFormatDesc&, int cols, int rows, size_t step)
{
    texture<T, 2, M>& w = const_cast<texture<T, 2, M>&>(t);
    w.data = p; w.cols = cols; w.rows = rows; w.step = step;
    return 0;
}
template<class T, cudaTextureReadMode M>
static inline int cudaBindTexture(size_t*, const texture<T, 1, M>&, const void*, const cudaChannelFormatDesc&, size_t) { return 0; }
static inline int cudaUnbindTexture(const textureReference*) { return 0; }
template<class T, cudaTextureReadMode M> static inline T tex2D(const texture<T, 2, M>& t, float x, float y)
{
    int ix = (int)floorf(x), iy = (int)floorf(y);
    ix = ix < 0 ? 0 : (ix >= t.cols ? t.cols - 1 : ix);
    iy = iy < 0 ? 0 : (iy >= t.rows ? t.rows - 1 : iy);
    return *(const T*)((const char*)t.data + (size_t)iy * t.step + (size_t)ix * sizeof(T));
}
