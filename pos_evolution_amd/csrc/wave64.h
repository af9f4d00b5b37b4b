// wave64.h -- reductions and the inclusive scan over the 64 lanes of a wave, by lane shuffles (no LDS, no barrier).
// Every lane of the wave must take part.  T: a 32- or 64-bit integer.
#pragma once
#include <hip/hip_runtime.h>

namespace posevo {

// sum over the wave, in every lane (xor butterfly)
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// maximum over the wave, in every lane
template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, (T)__shfl_xor(v, off, 64));
    return v;
}
// lane l gets the sum over lanes 0..l
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

}  // namespace posevo
