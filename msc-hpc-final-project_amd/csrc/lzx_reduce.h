// lzx_reduce.h -- the fixed-order block reduction every vector kernel closes the loop's partial sums with, and the one that
// writes a workgroup's partial (device code; include after lzx_spmv_body.h, which has wave_sum).
#pragma once

// out[workgroup] = the sum of s over the 256 threads of the workgroup, wavefronts added in order.  sh: >= 4 doubles of LDS.
__device__ __forceinline__ void block_partial(double s, double *sh, double *out)
{
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// The integer statistics of the graph routines: every lane gets the wavefront's sum / maximum ...
__device__ __forceinline__ ull wave_sum_u64(ull v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ ull wave_max_u64(ull v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const ull other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return v;
}

// ... and one thread the largest of the four wavefronts' maxima s[0 .. 4) (LDS, behind a barrier)
__device__ __forceinline__ ull block_max_u64(const ull *s)
{
    ull k = s[0];
    for (u32 w = 1; w < 4; ++w) k = s[w] > k ? s[w] : k;
    return k;
}

// Sum p[0..np) identically in every workgroup of a 256-thread launch. sh: >= 4 doubles of LDS.
__device__ __forceinline__ double block_sum_fixed_256(const double *p, u32 np, double *sh)
{
    // A thread's values are added in index order (the result does not depend on how the loads are scheduled), but they
    // are FETCHED eight at a time: one load per loop iteration was five dependent round trips for the ~1300 partials of
    // a blocked SpMV, at the head of every vector kernel (on the 1 M-vertex graph a third of k_lazy_update's 14 us).
    double s = 0.0;
    u32 i = threadIdx.x;
    for (; i + 7 * LZX_VEC_BLOCK < np; i += 8 * LZX_VEC_BLOCK) {
        double t[8];
#pragma unroll
        for (u32 u = 0; u < 8; ++u) t[u] = p[i + u * LZX_VEC_BLOCK];
#pragma unroll
        for (u32 u = 0; u < 8; ++u) s += t[u];
    }
    if (i < np) {   // up to seven more: clamped, unconditional loads
        double t[7];
#pragma unroll
        for (u32 u = 0; u < 7; ++u) {
            const u32 j = i + u * LZX_VEC_BLOCK;
            t[u] = p[j < np ? j : i];
        }
#pragma unroll
        for (u32 u = 0; u < 7; ++u)
            if (i + u * LZX_VEC_BLOCK < np) s += t[u];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    const double t = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return t;
}
