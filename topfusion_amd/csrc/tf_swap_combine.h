// tf_swap_combine.h -- CombineVoxelInformation, written once: the swapping engine's IntegrateGlobalIntoLocal
// (tf_swap.hip) writes it into the active block, the mesher's whole reading (tf_mesh_dev.h) forms the same
// bits on the fly for a block whose merge is still pending.
#pragma once
#include "tf_internal.h"

// CombineVoxelInformation (depth part): src = stored, dst = active; canonical arithmetic.  Voxels as
// their 32-bit words (sdf | w << 16 | pad << 24); the result keeps dst's top byte.
__device__ __forceinline__ unsigned sw_combine(unsigned src, unsigned dst, int maxW)
{
    const int oldW = (src >> 16) & 0xff, newW0 = (dst >> 16) & 0xff;
    if (oldW == 0) return dst;
    const float oldF = tf_short_to_float((short)(src & 0xffff)), newF0 = tf_short_to_float((short)(dst & 0xffff));
    float newF = (float)oldW * oldF + (float)newW0 * newF0;
    int newW = oldW + newW0;
    newF = newF / (float)newW;
    newW = newW < maxW ? newW : maxW;
    const short sdf = (short)(newF * 32767.0f);
    return (unsigned)(unsigned short)sdf | ((unsigned)(newW & 0xff) << 16) | (dst & 0xff000000u);
}
