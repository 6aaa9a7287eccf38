// rowreduce.h -- the wave / block reductions of the one-workgroup-per-row kernels (aux.hip: softmax / NLL rows; beam.hip:
// vocabulary top-k).  Shared so that a log-normaliser computed in either file is the same sequence of operations:
// xor-butterfly 32..1 inside each wave64, then the per-wave partials combined in ascending wave order.
#pragma once
#include <hip/hip_runtime.h>

namespace s2vt {

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
template <bool IS_MAX>
__device__ __forceinline__ float block_reduce(float v, float* sh)
{
    v = IS_MAX ? wave_max(v) : wave_sum(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    float r = sh[0];
    for (int i = 1; i < nw; ++i) r = IS_MAX ? fmaxf(r, sh[i]) : r + sh[i];
    return r;
}

}  // namespace s2vt
