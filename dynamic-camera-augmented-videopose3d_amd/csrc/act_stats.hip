// Per-layer activation statistics of the f16x3 calibration pass (vp3d_x3_calibrate).
//
// One HBM-bound grid-stride reduction over a layer's f32 output rows: 16-byte loads (four in
// flight per lane), per-lane partials in registers, a wave all-reduce on DPP and
// v_permlane{16,32}_swap, the four waves of a workgroup through 96 bytes of LDS, then one atomic
// per statistic per workgroup, spread over kActStatSlots accumulator lines (with all 2,048
// workgroups on one address the atomics, not HBM, set the time: 38 us for a 4 MB layer).  The
// grid is sized from the CU count (launch_act_stats), not from the rows, so a layer costs at
// most 8 workgroups x 3 atomics per CU.
//
// The three statistics (kernels.h ActStats) are order-independent but for the f64 sum of
// squares, whose products are exact (an f32 square has 48 significant bits) and whose sum
// differs between runs by f64 rounding only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace vp3d {
namespace {

constexpr int kStatThreads = 256;
constexpr int kStatWaves = kStatThreads / 64;
constexpr int kStatBlocksPerCU = 8;
constexpr unsigned kAbsMask = 0x7FFFFFFFu;
constexpr unsigned kSmallBits = 0x3E000000u;  // 2^-3: below it the split's lo half is an f16 subnormal

template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v) {
    return (unsigned)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, false);
}

// (x, y) = (v, v) -> after the swap one of them holds the partner half's / row's value in every
// lane (v_permlane32_swap: lanes 32-63 of x <-> lanes 0-31 of y; v_permlane16_swap: the odd
// 16-lane rows of x <-> the even ones of y).  v was written by VALU: 2 wait states first.
#define VP3D_SWAP32(x, y) asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y))
#define VP3D_SWAP16(x, y) asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y))

struct Partial {
    unsigned amax;          // max of |a| bit patterns
    unsigned small;         // count (a lane sees < 2^32 values: n / lanes, far below)
    double sumsq;
};

__device__ __forceinline__ Partial combine(const Partial& a, const Partial& b) {
    return Partial{a.amax > b.amax ? a.amax : b.amax, a.small + b.small, a.sumsq + b.sumsq};
}

__device__ __forceinline__ Partial from_words(unsigned m, unsigned c, unsigned lo, unsigned hi) {
    return Partial{m, c, __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo)};
}

template <int CTRL>
__device__ __forceinline__ Partial dpp_step(const Partial& p) {
    const unsigned long long q = __builtin_bit_cast(unsigned long long, p.sumsq);
    return combine(p, from_words(dpp_u32<CTRL>(p.amax), dpp_u32<CTRL>(p.small), dpp_u32<CTRL>((unsigned)q),
                                 dpp_u32<CTRL>((unsigned)(q >> 32))));
}

// every lane ends with the wave's total
__device__ __forceinline__ Partial wave_allreduce(Partial p) {
    p = dpp_step<0xB1>(p);   // quad_perm [1,0,3,2]: xor 1
    p = dpp_step<0x4E>(p);   // quad_perm [2,3,0,1]: xor 2
    p = dpp_step<0x141>(p);  // row_half_mirror: the other quad of the 8 lanes
    p = dpp_step<0x140>(p);  // row_mirror: the other 8 lanes of the 16-lane row
#pragma unroll
    for (int step = 0; step < 2; ++step) {
        const unsigned long long q = __builtin_bit_cast(unsigned long long, p.sumsq);
        unsigned w[4] = {p.amax, p.small, (unsigned)q, (unsigned)(q >> 32)};
        unsigned x[4], y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[i] = w[i];
            y[i] = w[i];
            if (step == 0)
                VP3D_SWAP16(x[i], y[i]);
            else
                VP3D_SWAP32(x[i], y[i]);
        }
        p = combine(from_words(x[0], x[1], x[2], x[3]), from_words(y[0], y[1], y[2], y[3]));
    }
    return p;
}

__device__ __forceinline__ void take(Partial& p, float v) {
    const unsigned b = __builtin_bit_cast(unsigned, v) & kAbsMask;
    p.amax = b > p.amax ? b : p.amax;
    p.small += (b != 0u && b < kSmallBits) ? 1u : 0u;
    p.sumsq += (double)v * (double)v;
}

__device__ __forceinline__ void take4(Partial& p, const float4& v) {
    take(p, v.x);
    take(p, v.y);
    take(p, v.z);
    take(p, v.w);
}

// a: 16-byte aligned; n4 float4 units, then `rest` (< 4) trailing floats
__global__ __launch_bounds__(kStatThreads) void act_stats_kernel(const float* __restrict__ a, int64_t n4, int rest,
                                                                 ActStats* __restrict__ out) {
    __shared__ Partial s_part[kStatWaves];
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const int64_t step = (int64_t)gridDim.x * kStatThreads;
    int64_t i = blockIdx.x * (int64_t)kStatThreads + threadIdx.x;
    Partial p{0u, 0u, 0.0};
    for (; i + 3 * step < n4; i += 4 * step) {
        const float4 v0 = a4[i], v1 = a4[i + step], v2 = a4[i + 2 * step], v3 = a4[i + 3 * step];
        take4(p, v0);
        take4(p, v1);
        take4(p, v2);
        take4(p, v3);
    }
    for (; i < n4; i += step) take4(p, a4[i]);
    if (blockIdx.x == 0 && (int)threadIdx.x < rest) take(p, a[4 * n4 + threadIdx.x]);

    p = wave_allreduce(p);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_part[wave] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
        Partial t = s_part[0];
#pragma unroll
        for (int w = 1; w < kStatWaves; ++w) t = combine(t, s_part[w]);
        ActStats* slot = out + (blockIdx.x % kActStatSlots);
        atomicMax(&slot->absmax_bits, t.amax);
        unsafeAtomicAdd(&slot->sumsq, t.sumsq);  // (global_atomic_add_f64, no compare-and-swap loop)
        atomicAdd(&slot->small, (unsigned long long)t.small);
    }
}

}  // namespace

hipError_t launch_act_stats(const float* a, int64_t n, ActStats* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (reinterpret_cast<uintptr_t>(a) & 15) return hipErrorInvalidValue;  // (the workspace rows are aligned)
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const int64_t n4 = n / 4;
    const int64_t want = std::max<int64_t>(1, (n4 + kStatThreads - 1) / kStatThreads);
    const unsigned blocks = (unsigned)std::min<int64_t>(want, (int64_t)std::max(cus, 1) * kStatBlocksPerCU);
    hipLaunchKernelGGL(act_stats_kernel, dim3(blocks), dim3(kStatThreads), 0, s, a, n4, (int)(n - 4 * n4), out);
    return hipGetLastError();
}

}  // namespace vp3d
