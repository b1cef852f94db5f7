// The StackedPoseLifter MLP (reference common/models/StackedPoseLifter.py:22-56) in one launch:
// Linear(2 J F -> H), ReLU, [Linear(H -> H), ReLU] x num_layers, Linear(H -> J F) on rows of
// [transformer prediction | FCN prediction]; eval mode, so every Dropout is the identity.
//
// A workgroup (4 waves) owns 16 MI rows (MI = 1, 2, 4).  Their activations live in two LDS
// buffers that swap roles after every layer and never go to HBM: the first layer's input is
// read straight from the two prediction tensors (no concat buffer), the last layer's output is
// written straight to y.  Layer widths are zero padded to 16 at pack time; a padded output
// column has zero weights and a zero bias, so it writes relu(0) = 0 and the next layer's padded
// K columns are zeros, not stale LDS.
//
// Exact f32: v_mfma_f32_16x16x4_f32, the k order of conv_gemm_f32 (a 16-deep step is 4 MFMAs
// s = 0..3, lane group c = lane >> 4 holding k = 16 kt + 4 c + s).  The order of an output's
// fmaf chain is therefore (kt, s, c) whatever the row tile, the row's place in it or the number
// of rows: a row's result depends on that row alone, bit for bit.
//
// The weights are packed on the host in B-operand order -- for column block jb and K-step kt the
// 64 lanes' four floats are one contiguous KiB -- and every wave reads its column blocks
// from global memory (L2: the whole network is under 4 MB and every workgroup reads all of it),
// kPF K-steps ahead of the MFMAs that use them.  Wave w takes column blocks w, w + 4, w + 8,
// w + 12 of a layer per pass, so the 4-block output layer (51 -> 64 columns) still uses 4 waves.
#include <initializer_list>

#include "kernels.h"

namespace vp3d {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kNJ = 4;  // column blocks per wave per pass
constexpr int kPF = 4;  // K-steps of weights in flight per wave

// acc[i][j] += in[rows 16 i ..][:] . W[column block jb0 + 4 j]^T over the layer's nk K-steps
template <int MI, int NJ>
__device__ __forceinline__ void layer_tile(const float* in, int ld, const float* W, int nk, int jb0, int lane,
                                           f32x4 (&acc)[MI][kNJ]) {
    const f32x4* wp[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) wp[j] = (const f32x4*)W + (size_t)(jb0 + 4 * j) * nk * 64 + lane;
    const float* const arow = in + (lane & 15) * ld + 4 * (lane >> 4);
    f32x4 bw[kPF][NJ];
    auto load_step = [&](int kt, f32x4 (&b)[NJ]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j] = wp[j][(size_t)kt * 64];
    };
#pragma unroll
    for (int d = 0; d < kPF; ++d)
        if (d < nk) load_step(d, bw[d]);
    for (int kt0 = 0; kt0 < nk; kt0 += kPF) {
#pragma unroll
        for (int d = 0; d < kPF; ++d) {
            const int kt = kt0 + d;
            if (kt < nk) {
                f32x4 a[MI];
#pragma unroll
                for (int i = 0; i < MI; ++i) a[i] = *(const f32x4*)(arow + i * 16 * ld + 16 * kt);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s], bw[d][j][s], acc[i][j], 0, 0, 0);
                if (kt + kPF < nk) load_step(kt + kPF, bw[d]);
            }
        }
    }
}

template <int MI>
__global__ __launch_bounds__(kThreads) void stacked_mlp_kernel(StackedParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int RT = 16 * MI;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane >> 4, r = lane & 15;
    const int ld = p.ld, D = p.D;
    const int64_t m0 = (int64_t)blockIdx.x * RT;

    // layer-0 input: [transformer | FCN | zeros to Kp[0]] (StackedPoseLifter.py:46-49); rows past
    // n_rows are zeros and are never stored
    float* in = smem;
    float* out = smem + RT * ld;
    const int K0 = p.Kp[0];
    for (int idx = tid; idx < RT * K0; idx += kThreads) {
        const int row = idx / K0, col = idx - row * K0;
        const int64_t m = m0 + row;
        float v = 0.f;
        if (m < p.n_rows) {
            if (col < D)
                v = p.ya[m * D + col];
            else if (col < 2 * D)
                v = p.yb[m * D + (col - D)];
        }
        in[row * ld + col] = v;
    }
    __syncthreads();

    for (int l = 0; l < p.n_lin; ++l) {
        const int nk = p.Kp[l] >> 4, NB = p.Np[l] >> 4;
        const bool last = l + 1 == p.n_lin;
        const float* const W = p.w + p.w_off[l];
        const float* const bias = p.w + p.b_off[l];
        for (int jb0 = wid; jb0 < NB; jb0 += 4 * kNJ) {
            const int nj = min(kNJ, (NB - jb0 + 3) >> 2);  // wave-uniform
            f32x4 acc[MI][kNJ];
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < kNJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (nj == 4)
                layer_tile<MI, 4>(in, ld, W, nk, jb0, lane, acc);
            else if (nj == 3)
                layer_tile<MI, 3>(in, ld, W, nk, jb0, lane, acc);
            else if (nj == 2)
                layer_tile<MI, 2>(in, ld, W, nk, jb0, lane, acc);
            else
                layer_tile<MI, 1>(in, ld, W, nk, jb0, lane, acc);
            // accumulator layout: column 16 jb + r, rows 16 i + 4 c + q
#pragma unroll
            for (int j = 0; j < kNJ; ++j) {
                if (j >= nj) break;
                const int col = 16 * (jb0 + 4 * j) + r;
                const float b = bias[col];
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int row = 16 * i + 4 * c + q;
                        const float v = acc[i][j][q] + b;
                        if (!last) {
                            out[row * ld + col] = v < 0.f ? 0.f : v;  // ReLU (a NaN stays a NaN)
                        } else if (col < D && m0 + row < p.n_rows) {
                            p.y[(m0 + row) * D + col] = v;
                        }
                    }
            }
        }
        // every wave has read `in` and written its columns of `out`
        __syncthreads();
        float* t = in;
        in = out;
        out = t;
    }
}

template <int MI>
const void* kernel_of() {
    return (const void*)&stacked_mlp_kernel<MI>;
}

}  // namespace

int stacked_mlp_lds_bytes(int mi, int ld) { return 2 * 16 * mi * ld * (int)sizeof(float); }

hipError_t stacked_mlp_prepare() {
    for (const void* f : {kernel_of<1>(), kernel_of<2>(), kernel_of<4>()}) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kStackedMaxLds);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_stacked_mlp(const StackedParams& p, int mi, hipStream_t s) {
    if (p.n_rows <= 0 || (mi != 1 && mi != 2 && mi != 4)) return hipErrorInvalidValue;
    const int64_t nwg = (p.n_rows + 16 * mi - 1) / (16 * mi);
    if (nwg > 0x7FFFFFFF) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nwg), block(kThreads);
    const size_t lds = (size_t)stacked_mlp_lds_bytes(mi, p.ld);
    if (mi == 4)
        hipLaunchKernelGGL(stacked_mlp_kernel<4>, grid, block, lds, s, p);
    else if (mi == 2)
        hipLaunchKernelGGL(stacked_mlp_kernel<2>, grid, block, lds, s, p);
    else
        hipLaunchKernelGGL(stacked_mlp_kernel<1>, grid, block, lds, s, p);
    return hipGetLastError();
}

}  // namespace vp3d
