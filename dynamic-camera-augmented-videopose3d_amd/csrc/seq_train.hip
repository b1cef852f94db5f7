// Train-mode kernels of the CoupledLSTM trajectory lifter (reference CamLSTM.py:47-129 in
// train mode, driven by run.py:451-487): what one optimisation step needs beyond the f32
// GEMM (layer 0's input projection), the split weight-gradient GEMM and the column sums
// (train.hip).
//
//   lstm_train_fwd_kernel   the stacked nn.LSTM recurrence of a tile of windows, persistent
//                           over all time steps like the eval kernel (seq_lifter.hip
//                           lstm_kernel), storing per (window, step, layer) the activated
//                           gates, the cell state and the hidden state, and applying
//                           nn.LSTM's inter-layer dropout
//   lstm_bptt_kernel        the backward through time of a tile of windows in one launch:
//                           t = T-1 .. 0, layers top to bottom; dc and dh live in registers,
//                           a step's gate-gradient rows da in LDS for the two products
//                           da W_hh (-> dh of step t-1) and da W_ih (-> dh of the layer below)
//   head kernels            the MLP head on B rows: Linear, BatchNorm (batch statistics) +
//                           LeakyReLU + Dropout forward and backward
//
// f32 throughout; every sum runs in a fixed order (no atomics), so a step is reproducible
// bit for bit.
#include <climits>

#include "dropout_hash.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace vp3d {
namespace {

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// acc[q][i] += sum_k x[i][k] * WT[k][q*H + u], k ascending (WT rows of 4H, x rows of H in LDS)
template <int H, int NWH>
__device__ __forceinline__ void gate_gemv(float (&acc)[4][NWH], const float* __restrict__ WT, const float* x, int u) {
    constexpr int G = 4 * H;
    for (int k = 0; k < H; k += 4) {
        float wv[4][4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int q = 0; q < 4; ++q) wv[kk][q] = WT[(k + kk) * G + q * H + u];
#pragma unroll
        for (int i = 0; i < NWH; ++i) {
            const float4 xv = *(const float4*)&x[i * H + k];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[q][i] = fmaf(xv.x, wv[0][q], acc[q][i]);
                acc[q][i] = fmaf(xv.y, wv[1][q], acc[q][i]);
                acc[q][i] = fmaf(xv.z, wv[2][q], acc[q][i]);
                acc[q][i] = fmaf(xv.w, wv[3][q], acc[q][i]);
            }
        }
    }
}

// Thread (u, half) owns hidden unit u of windows [half*NWH, half*NWH + NWH) of the tile: that
// unit's four gates and cell state in every layer, as in the eval kernel.  The tile's hidden
// states (one buffer per layer, rewritten behind a barrier) and the dropped output of the layer
// below live in LDS.
template <int H, int NW, int MAXL>
__global__ __launch_bounds__(2 * H) void lstm_train_fwd_kernel(LstmTrainParams p) {
    constexpr int NWH = NW / 2;
    constexpr int G = 4 * H;
    __shared__ __attribute__((aligned(16))) float hs[MAXL][NW][H];
    __shared__ __attribute__((aligned(16))) float hd[NW][H];
    const int u = threadIdx.x % H;
    const int half = threadIdx.x / H;
    const int w0 = blockIdx.x * NW + half * NWH;
    const int T = p.T;
    for (int e = threadIdx.x; e < MAXL * NW * H; e += blockDim.x) (&hs[0][0][0])[e] = 0.f;
    for (int e = threadIdx.x; e < NW * H; e += blockDim.x) (&hd[0][0])[e] = 0.f;
    float c[MAXL][NWH];
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
#pragma unroll
        for (int i = 0; i < NWH; ++i) c[l][i] = 0.f;
    // the zero rows in front of every window's states
    for (int l = 0; l < p.L; ++l)
        for (int i = 0; i < NWH; ++i) {
            const int w = w0 + i;
            if (w < p.B) {
                const int64_t r = ((int64_t)l * p.B + w) * (T + 1) * H + u;
                p.cs[r] = 0.f;
                p.hs[r] = 0.f;
            }
        }
    __syncthreads();
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int l = 0; l < MAXL; ++l) {
            if (l >= p.L) continue;
            float acc[4][NWH];
#pragma unroll
            for (int i = 0; i < NWH; ++i) {
                const int w = w0 + i;
                if (l == 0) {
                    const float* g = p.gin + ((int64_t)(w < p.B ? w : 0) * T + t) * G;
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q][i] = g[q * H + u];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q][i] = p.bias[l][q * H + u];
                }
            }
            if (l > 0) gate_gemv<H, NWH>(acc, p.wih_t[l], &hd[half * NWH][0], u);
            gate_gemv<H, NWH>(acc, p.whh_t[l], &hs[l][half * NWH][0], u);
            __syncthreads();  // every read of hs[l] and hd is done
#pragma unroll
            for (int i = 0; i < NWH; ++i) {
                const int w = w0 + i;
                const float ig = sigm(acc[0][i]), fg = sigm(acc[1][i]);
                const float gg = tanhf(acc[2][i]), og = sigm(acc[3][i]);
                const float cc = fg * c[l][i] + ig * gg;
                c[l][i] = cc;
                const float hv = og * tanhf(cc);
                hs[l][half * NWH + i][u] = hv;
                if (w < p.B) {
                    float* g = p.gates + (((int64_t)l * p.B + w) * T + t) * G;
                    g[u] = ig;
                    g[H + u] = fg;
                    g[2 * H + u] = gg;
                    g[3 * H + u] = og;
                    const int64_t r = (((int64_t)l * p.B + w) * (T + 1) + t + 1) * H + u;
                    p.cs[r] = cc;
                    p.hs[r] = hv;
                }
                if (l + 1 < p.L) {
                    float dv = hv;
                    if (p.thresh != (1ull << 32))
                        dv = drop_keep(p.seed, l, ((int64_t)w * T + t) * H + u, p.thresh) ? hv * p.dscale : 0.f;
                    hd[half * NWH + i][u] = dv;
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int l = 0; l < MAXL; ++l) {
        if (l != p.L - 1) continue;
#pragma unroll
        for (int i = 0; i < NWH; ++i) {
            const int w = w0 + i;
            if (w < p.B) p.hlast[(int64_t)w * H + u] = hs[l][half * NWH + i][u];
        }
    }
}

// Backward through time of a tile of BPTT_NW windows.  Thread (u, half) owns unit u of 8
// windows in every layer: dc and dh of that unit in registers.  Per (t, l): da from the stored
// gates and cell states into LDS and back over the stored gates, then
//   dh[l]    = da W_hh[l]                       (the recurrent path into step t-1)
//   dh[l-1] += mask(da W_ih[l]) / (1-p)         (the layer below at the same step)
// each a reduction over the 4H gate columns in ascending order, W rows of H read coalesced.
constexpr int BPTT_NW = 16;

template <int H, int NWH>
__device__ __forceinline__ void da_gemv(float (&acc)[NWH], const float* __restrict__ W, const float* da, int u) {
    constexpr int G = 4 * H;
    for (int n = 0; n < G; n += 4) {
        float wv[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) wv[kk] = W[(n + kk) * H + u];
#pragma unroll
        for (int i = 0; i < NWH; ++i) {
            const float4 dv = *(const float4*)&da[i * G + n];
            acc[i] = fmaf(dv.x, wv[0], acc[i]);
            acc[i] = fmaf(dv.y, wv[1], acc[i]);
            acc[i] = fmaf(dv.z, wv[2], acc[i]);
            acc[i] = fmaf(dv.w, wv[3], acc[i]);
        }
    }
}

template <int H, int MAXL>
__global__ __launch_bounds__(2 * H) void lstm_bptt_kernel(LstmBpttParams p) {
    constexpr int NW = BPTT_NW, NWH = NW / 2;
    constexpr int G = 4 * H;
    __shared__ __attribute__((aligned(16))) float das[NW][G];
    const int u = threadIdx.x % H;
    const int half = threadIdx.x / H;
    const int w0 = blockIdx.x * NW + half * NWH;
    const int T = p.T;
    float dh[MAXL][NWH], dc[MAXL][NWH];
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
#pragma unroll
        for (int i = 0; i < NWH; ++i) {
            const int w = w0 + i;
            dh[l][i] = (l == p.L - 1 && w < p.B) ? p.dhlast[(int64_t)w * H + u] : 0.f;
            dc[l][i] = 0.f;
        }
    for (int t = T - 1; t >= 0; --t) {
#pragma unroll
        for (int l = MAXL - 1; l >= 0; --l) {
            if (l >= p.L) continue;
#pragma unroll
            for (int i = 0; i < NWH; ++i) {
                const int w = w0 + i;
                float ai = 0.f, af = 0.f, ag = 0.f, ao = 0.f;
                if (w < p.B) {
                    float* g = p.gates + (((int64_t)l * p.B + w) * T + t) * G;
                    const float ig = g[u], fg = g[H + u], gg = g[2 * H + u], og = g[3 * H + u];
                    const int64_t r = (((int64_t)l * p.B + w) * (T + 1) + t) * H + u;
                    const float cprev = p.cs[r], cc = p.cs[r + H];
                    const float tc = tanhf(cc);
                    const float dhv = dh[l][i];
                    const float dcv = dc[l][i] + dhv * og * (1.0f - tc * tc);
                    dc[l][i] = dcv * fg;
                    ai = dcv * gg * (ig * (1.0f - ig));
                    af = dcv * cprev * (fg * (1.0f - fg));
                    ag = dcv * ig * (1.0f - gg * gg);
                    ao = dhv * tc * (og * (1.0f - og));
                    g[u] = ai;
                    g[H + u] = af;
                    g[2 * H + u] = ag;
                    g[3 * H + u] = ao;
                }
                float* d = &das[half * NWH + i][0];
                d[u] = ai;
                d[H + u] = af;
                d[2 * H + u] = ag;
                d[3 * H + u] = ao;
            }
            __syncthreads();
            if (t > 0) {
                float acc[NWH];
#pragma unroll
                for (int i = 0; i < NWH; ++i) acc[i] = 0.f;
                da_gemv<H, NWH>(acc, p.whh[l], &das[half * NWH][0], u);
#pragma unroll
                for (int i = 0; i < NWH; ++i) dh[l][i] = acc[i];
            }
            if (l > 0) {
                float acc[NWH];
#pragma unroll
                for (int i = 0; i < NWH; ++i) acc[i] = 0.f;
                da_gemv<H, NWH>(acc, p.wih[l], &das[half * NWH][0], u);
#pragma unroll
                for (int i = 0; i < NWH; ++i) {
                    float dx = acc[i];
                    if (p.thresh != (1ull << 32))
                        dx = drop_keep(p.seed, l - 1, ((int64_t)(w0 + i) * T + t) * H + u, p.thresh) ? dx * p.dscale
                                                                                                     : 0.f;
                    // l - 1 >= 0 here; the index is clamped for the unrolled l = 0 copy the branch removes
                    dh[l > 0 ? l - 1 : 0][i] = dh[l > 0 ? l - 1 : 0][i] + dx;
                }
            }
            __syncthreads();  // das is rewritten by the next (t, l)
        }
    }
}

__global__ void lstm_drop_rows_kernel(const float* __restrict__ hs, int64_t rows, int T, int H, float dscale,
                                      uint64_t seed, uint64_t thresh, int site, float* __restrict__ out) {
    const int64_t total = rows * H;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = e / H;
        const int u = (int)(e - m * H);
        const int64_t b = m / T, t = m - b * T;
        float v = hs[(b * (T + 1) + t + 1) * H + u];
        if (thresh != (1ull << 32)) v = drop_keep(seed, site, e, thresh) ? v * dscale : 0.f;
        out[e] = v;
    }
}

__global__ void vec_add_kernel(const float* __restrict__ a, const float* __restrict__ b, int n,
                               float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}

// Y[m][n] = bias[n] + sum_k X[m][k] W[n][k], k ascending.  16 x 16 outputs per workgroup, the
// operands staged through LDS 16 columns at a time.
__global__ __launch_bounds__(256) void head_linear_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                          const float* __restrict__ bias, int M, int N, int K,
                                                          float* __restrict__ Y) {
    __shared__ float xs[16][17], ws[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m0 = blockIdx.y * 16, n0 = blockIdx.x * 16;
    float acc = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {
        xs[ty][tx] = (m0 + ty < M && k0 + tx < K) ? X[(int64_t)(m0 + ty) * K + k0 + tx] : 0.f;
        ws[ty][tx] = (n0 + ty < N && k0 + tx < K) ? W[(int64_t)(n0 + ty) * K + k0 + tx] : 0.f;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = fmaf(xs[ty][k], ws[tx][k], acc);
        __syncthreads();
    }
    if (m0 + ty < M && n0 + tx < N) Y[(int64_t)(m0 + ty) * N + n0 + tx] = acc + bias[n0 + tx];
}

// dX[m][k] = sum_n dY[m][n] W[n][k], n ascending
__global__ __launch_bounds__(256) void head_linear_dgrad_kernel(const float* __restrict__ dY,
                                                                const float* __restrict__ W, int M, int N, int K,
                                                                float* __restrict__ dX) {
    __shared__ float ds[16][17], ws[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m0 = blockIdx.y * 16, k0 = blockIdx.x * 16;
    float acc = 0.f;
    for (int n0 = 0; n0 < N; n0 += 16) {
        ds[ty][tx] = (m0 + ty < M && n0 + tx < N) ? dY[(int64_t)(m0 + ty) * N + n0 + tx] : 0.f;
        ws[ty][tx] = (n0 + ty < N && k0 + tx < K) ? W[(int64_t)(n0 + ty) * K + k0 + tx] : 0.f;
        __syncthreads();
#pragma unroll
        for (int n = 0; n < 16; ++n) acc = fmaf(ds[ty][n], ws[n][tx], acc);
        __syncthreads();
    }
    if (m0 + ty < M && k0 + tx < K) dX[(int64_t)(m0 + ty) * K + k0 + tx] = acc;
}

__global__ void bn_leaky_fwd_kernel(const float* __restrict__ Z, int64_t total, int C, const float* __restrict__ alpha,
                                    const float* __restrict__ shift, float slope, float dscale, uint64_t seed,
                                    uint64_t thresh, int site, float* __restrict__ Y) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        float v = Z[e] * alpha[c];
        v = v + shift[c];
        v = v > 0.f ? v : v * slope;
        if (thresh != (1ull << 32)) v = drop_keep(seed, site, e, thresh) ? v * dscale : 0.f;
        Y[e] = v;
    }
}

// gradient wrt the BatchNorm output of element e: through the dropout and the LeakyReLU
__device__ __forceinline__ float leaky_grad(float d, float z, float al, float sh, float slope, float dscale,
                                            uint64_t seed, uint64_t thresh, int site, int64_t e) {
    const float y = z * al + sh;
    float g = y > 0.f ? d : d * slope;
    if (thresh != (1ull << 32)) g = drop_keep(seed, site, e, thresh) ? g * dscale : 0.f;
    return g;
}

// one wave per channel: sum g and sum g (z - mean) over the M rows in f64 (lane j takes rows
// j, j + 64, ...; the lanes are combined in a fixed butterfly), then the coefficients of
// bn_bwd_finalize_kernel (train.hip)
__global__ __launch_bounds__(64) void bn_leaky_bwd_reduce_kernel(const float* __restrict__ dO,
                                                                 const float* __restrict__ Z, int M, int C,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ alpha,
                                                                 const float* __restrict__ shift,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, float slope,
                                                                 float dscale, uint64_t seed, uint64_t thresh, int site,
                                                                 float* __restrict__ coef, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta) {
    const int c = blockIdx.x;
    const float al = alpha[c], sh = shift[c], mu = mean[c];
    double a = 0, b = 0;
    for (int m = threadIdx.x; m < M; m += 64) {
        const int64_t e = (int64_t)m * C + c;
        const float z = Z[e];
        const float g = leaky_grad(dO[e], z, al, sh, slope, dscale, seed, thresh, site, e);
        a += g;
        b += (double)g * (double)(z - mu);
    }
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if (threadIdx.x == 0) {
        const double is = invstd[c];
        if (dgamma) dgamma[c] = (float)(b * is);
        if (dbeta) dbeta[c] = (float)a;
        coef[c] = (float)(a / (double)M);
        coef[C + c] = (float)(b * is * is / (double)M);
        coef[2 * C + c] = (float)(is * (double)gamma[c]);
    }
}

__global__ void bn_leaky_bwd_apply_kernel(const float* __restrict__ dO, const float* __restrict__ Z, int64_t total,
                                          int C, const float* __restrict__ alpha, const float* __restrict__ shift,
                                          const float* __restrict__ mean, const float* __restrict__ coef, float slope,
                                          float dscale, uint64_t seed, uint64_t thresh, int site,
                                          float* __restrict__ dZ) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const float z = Z[e];
        const float g = leaky_grad(dO[e], z, alpha[c], shift[c], slope, dscale, seed, thresh, site, e);
        const float v = (g - coef[c]) - (z - mean[c]) * coef[C + c];
        dZ[e] = v * coef[2 * C + c];
    }
}

inline int grid1(int64_t n, int per = 256) {
    int64_t g = (n + per - 1) / per;
    if (g < 1) g = 1;
    return (int)(g < 65536 ? g : 65536);
}

}  // namespace

hipError_t launch_lstm_train_fwd(const LstmTrainParams& p, hipStream_t s) {
    if (p.L < 1 || p.L > 4 || p.B < 1 || p.T < 1) return hipErrorInvalidValue;
    if (p.H == 128 && p.L <= 2) {
        hipLaunchKernelGGL((lstm_train_fwd_kernel<128, 32, 2>), dim3((p.B + 31) / 32), dim3(256), 0, s, p);
        return hipGetLastError();
    }
    const dim3 grid((p.B + 15) / 16);
    switch (p.H) {
        case 64: hipLaunchKernelGGL((lstm_train_fwd_kernel<64, 16, 4>), grid, dim3(128), 0, s, p); break;
        case 128: hipLaunchKernelGGL((lstm_train_fwd_kernel<128, 16, 4>), grid, dim3(256), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_lstm_bptt(const LstmBpttParams& p, hipStream_t s) {
    if (p.L < 1 || p.L > 4 || p.B < 1 || p.T < 1) return hipErrorInvalidValue;
    const dim3 grid((p.B + BPTT_NW - 1) / BPTT_NW);
    if (p.H == 128 && p.L <= 2)
        hipLaunchKernelGGL((lstm_bptt_kernel<128, 2>), grid, dim3(256), 0, s, p);
    else if (p.H == 128)
        hipLaunchKernelGGL((lstm_bptt_kernel<128, 4>), grid, dim3(256), 0, s, p);
    else if (p.H == 64)
        hipLaunchKernelGGL((lstm_bptt_kernel<64, 4>), grid, dim3(128), 0, s, p);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_lstm_drop_rows(const float* hs, int B, int T, int H, float p, uint64_t seed, int site, float* out,
                                 hipStream_t s) {
    const int64_t rows = (int64_t)B * T;
    hipLaunchKernelGGL(lstm_drop_rows_kernel, dim3(grid1(rows * H)), dim3(256), 0, s, hs, rows, T, H, keep_scale(p),
                       seed, keep_threshold(p), site, out);
    return hipGetLastError();
}

hipError_t launch_vec_add(const float* a, const float* b, int n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(vec_add_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, b, n, out);
    return hipGetLastError();
}

hipError_t launch_head_linear(const float* X, const float* W, const float* bias, int M, int N, int K, float* Y,
                              hipStream_t s) {
    hipLaunchKernelGGL(head_linear_kernel, dim3((N + 15) / 16, (M + 15) / 16), dim3(256), 0, s, X, W, bias, M, N, K, Y);
    return hipGetLastError();
}

hipError_t launch_head_linear_dgrad(const float* dY, const float* W, int M, int N, int K, float* dX, hipStream_t s) {
    hipLaunchKernelGGL(head_linear_dgrad_kernel, dim3((K + 15) / 16, (M + 15) / 16), dim3(256), 0, s, dY, W, M, N, K,
                       dX);
    return hipGetLastError();
}

hipError_t launch_bn_leaky_fwd(const float* Z, int M, int C, const float* alpha, const float* shift, float slope,
                               float p, uint64_t seed, int site, float* Y, hipStream_t s) {
    const int64_t total = (int64_t)M * C;
    hipLaunchKernelGGL(bn_leaky_fwd_kernel, dim3(grid1(total)), dim3(256), 0, s, Z, total, C, alpha, shift, slope,
                       keep_scale(p), seed, keep_threshold(p), site, Y);
    return hipGetLastError();
}

hipError_t launch_bn_leaky_bwd(const float* dO, const float* Z, int M, int C, const float* gamma, const float* alpha,
                               const float* shift, const float* mean, const float* invstd, float slope, float p,
                               uint64_t seed, int site, float* coef, float* dgamma, float* dbeta, float* dZ,
                               hipStream_t s) {
    const float dscale = keep_scale(p);
    const uint64_t thresh = keep_threshold(p);
    hipLaunchKernelGGL(bn_leaky_bwd_reduce_kernel, dim3(C), dim3(64), 0, s, dO, Z, M, C, gamma, alpha, shift, mean,
                       invstd, slope, dscale, seed, thresh, site, coef, dgamma, dbeta);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t total = (int64_t)M * C;
    hipLaunchKernelGGL(bn_leaky_bwd_apply_kernel, dim3(grid1(total)), dim3(256), 0, s, dO, Z, total, C, alpha, shift,
                       mean, coef, slope, dscale, seed, thresh, site, dZ);
    return hipGetLastError();
}

}  // namespace vp3d
