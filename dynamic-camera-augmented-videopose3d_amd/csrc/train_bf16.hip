// bf16 mixed-precision training (vp3d_trainer_set_compute(VP3D_DTYPE_BF16)): the weight
// gradient of the block convolutions on v_mfma_f32_16x16x32_bf16, and the row copies behind
// the vp3d_train_read test hook.  The 16-bit operand copies come out of the element-wise passes
// of train.hip; forward and data gradient run on the 16-bit conv GEMMs (conv_gemm*.hip).
//
//   part[s][n][k] = sum_{m in split s} dZ[dzrow(m)][n] * X[src(m) + tap*dil][c],  k = tap*cin + c
//
// the contract of wgrad_f32_kernel (train.hip) with bf16 operand rows: the same 128 x 128 tiles,
// row splits, taps, stride, dilation, window boundaries and tails; f32 accumulation; the same
// deterministic split reduce (wgrad_reduce_kernel).
//
// The contraction index is the row m and both operands are m-major in memory, so both MFMA
// operands are COLUMN reads of row-major tiles.  A stage holds 64 rows of the dZ tile and of the
// gathered X tile as plain bf16 rows of 128 elements (256 bytes), and ds_read_b64_tr_b16 fetches
// the fragments: per 16-lane group it reads a block of 4 rows x 16 columns and hands lane i
// column i, so two reads (rows 8g .. 8g+3 and 8g+4 .. 8g+7 for lane group g) give a lane the 8
// consecutive k = 8g .. 8g+7 of its column that the 16x16x32 MFMA wants, for A and B alike.
//
// LDS image (per operand and buffer: 64 rows x 256 bytes): the 16-byte chunk ch (0..15) of row r
// sits at byte 256 r + 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))).  A 32-lane half of a
// transposed read takes two blocks 8 rows apart in the same 16 columns: rows r0 + q and
// r0 + 8 + q (q = 0..3), chunks c0 and c0 + 1, 8 bytes each.  The XOR puts q into chunk bits
// 2-3 and the two blocks' (r >> 2) & 3, which differ by 2, into bit 1; the chunk pair is bit 0:
// 16 different chunks x 2 halves of 8 bytes = all 64 banks once, conflict free.  A row's two
// 8-byte halves stay inside their 16-byte chunk, so lane 4q + p of a group addresses
// chunk' (c0 + (p >> 1)) ^ x, byte 8 (p & 1) -- the XOR is applied to the chunk index, never to
// `base + 8 p`.  Every address is a multiple of 8.  Rows past the split's end are stored as
// zero rows and columns past N / K as zero chunks, so every lane of every read is in bounds with
// the whole wave active (the transposed read needs full EXEC: pad, don't mask).
#include "kernels.h"

namespace vp3d {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4_ptr;

constexpr int WB_T = 128;              // tile edge (n and k)
constexpr int WB_R = 64;               // rows per stage (two MFMA k-steps of 32)
constexpr int WB_TILE = WB_R * 256;    // bytes of one operand's stage

__device__ __forceinline__ int wb_off(int row, int ch) {
    return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

__global__ __launch_bounds__(256) void wgrad_bf16_kernel(WgradParams p) {
    __shared__ __attribute__((aligned(16))) char sm[2][2][WB_TILE];  // [buf][dZ, X]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ntn = (p.N + WB_T - 1) / WB_T;
    const int tile_n = blockIdx.x % ntn, tile_k = blockIdx.x / ntn;
    const int n0 = tile_n * WB_T, k0 = tile_k * WB_T;
    const int64_t mb = (int64_t)blockIdx.y * p.rows_per_split;
    const int64_t me = min((int64_t)p.M, mb + p.rows_per_split);
    const __bf16* const dZ = (const __bf16*)p.dZ;
    const __bf16* const X = (const __bf16*)p.X;

    // loader: thread -> rows lr + 16 i (i = 0..3), the 16-byte chunk lc of both tiles
    // (N % 8 == 0 and cin % 8 == 0: a chunk is whole or empty and lies inside one tap)
    const int lr = tid >> 4, lc = tid & 15;
    const bool nval = n0 + lc * 8 < p.N;
    const int kk = k0 + lc * 8;
    const bool kval = kk < p.K;
    const int tapv = kval ? kk / p.cin : 0, cv = kval ? kk - tapv * p.cin : 0;
    u32x4 ra[4], rb[4];

    auto gload = [&](int64_t m0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t m = m0 + lr + 16 * i;
            const bool mv = m < me;
            int64_t b = 0, t = 0;
            if (mv) {
                b = m / p.T_out;
                t = m - b * p.T_out;
            }
            const __bf16* dzr = dZ + (b * p.dz_T + t + p.dz_off) * (int64_t)p.ldz + n0 + lc * 8;
            const __bf16* xr = X + (b * p.T_in + t * p.stride + (int64_t)tapv * p.dil) * p.cin + cv;
            ra[i] = (mv && nval) ? *(const u32x4*)dzr : u32x4{0u, 0u, 0u, 0u};
            rb[i] = (mv && kval) ? *(const u32x4*)xr : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = wb_off(lr + 16 * i, lc);
            *(u32x4*)&sm[buf][0][o] = ra[i];
            *(u32x4*)&sm[buf][1][o] = rb[i];
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wn = (wid >> 1) * 64, wk = (wid & 1) * 64;
    const int fr = lane >> 4, fc = lane & 15;
    // transposed-read addresses of k-step 0: lane 4q + pp of group g reads row 8g + 4h + q,
    // chunk (c0 + (pp >> 1)) ^ x, byte 8 (pp & 1); k-step 1 is 32 rows = 8192 bytes further
    // (32 rows on, r & 3 and (r >> 2) & 3 are the same)
    const int q = fc >> 2, pp = fc & 3;
    int a_addr[2][4], b_addr[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = 8 * fr + 4 * h + q;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a_addr[h][i] = wb_off(r, (wn >> 3) + 2 * i + (pp >> 1)) + 8 * (pp & 1);
            b_addr[h][i] = wb_off(r, (wk >> 3) + 2 * i + (pp >> 1)) + 8 * (pp & 1);
        }
    }

    if (mb < me) {
        gload(mb);
        lstore(0);
    }
    __syncthreads();
    int cur = 0;
    for (int64_t m0 = mb; m0 < me; m0 += WB_R) {
        const bool more = m0 + WB_R < me;
        if (more) gload(m0 + WB_R);
        const char* As = sm[cur][0];
        const char* Bs = sm[cur][1];
#pragma unroll
        for (int s = 0; s < WB_R / 32; ++s) {
            bf16x8 af[4], bfr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(As + s * 8192 + a_addr[0][i]));
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(As + s * 8192 + a_addr[1][i]));
                af[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(Bs + s * 8192 + b_addr[0][j]));
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(Bs + s * 8192 + b_addr[1][j]));
                bfr[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        if (more) lstore(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // D[n = 4 (lane / 16) + r][k = lane % 16] per 16 x 16 block, as wgrad_f32_kernel stores it
    float* out = p.part + (int64_t)blockIdx.y * p.N * (int64_t)p.K;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wn + i * 16 + fr * 4 + r;
                const int k = k0 + wk + j * 16 + fc;
                if (n < p.N && k < p.K) out[(int64_t)n * p.K + k] = acc[i][j][r];
            }
}

template <typename ST>
__global__ void rows_to_f32_kernel(const ST* __restrict__ src, int64_t M, int C, int T_out, int src_T, int src_off,
                                   float* __restrict__ out) {
    const int64_t total = M * C;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = e / C;
        const int c = (int)(e - m * C);
        const int64_t b = m / T_out, t = m - b * T_out;
        out[e] = (float)src[(b * src_T + t + src_off) * C + c];
    }
}

}  // namespace

hipError_t launch_wgrad_bf16_tiles(const WgradParams& p0, int S, hipStream_t s) {
    if (p0.N % 8 != 0 || p0.cin % 8 != 0 || p0.ldz % 8 != 0 || (reinterpret_cast<uintptr_t>(p0.dZ) & 15) ||
        (reinterpret_cast<uintptr_t>(p0.X) & 15))
        return hipErrorInvalidValue;
    WgradParams p = p0;
    const int64_t rps = (p.M + S - 1) / S;
    p.rows_per_split = (rps + WB_R - 1) / WB_R * WB_R;
    const int tiles = ((p.N + WB_T - 1) / WB_T) * ((p.K + WB_T - 1) / WB_T);
    hipLaunchKernelGGL(wgrad_bf16_kernel, dim3(tiles, S), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_rows_to_f32(const void* src, bool src_bf16, int64_t M, int C, int T_out, int src_T, int src_off,
                              float* out, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    int64_t g = (M * C + 255) / 256;
    if (g > 65536) g = 65536;
    if (src_bf16)
        hipLaunchKernelGGL(rows_to_f32_kernel<__bf16>, dim3((unsigned)g), dim3(256), 0, s, (const __bf16*)src, M, C,
                           T_out, src_T, src_off, out);
    else
        hipLaunchKernelGGL(rows_to_f32_kernel<float>, dim3((unsigned)g), dim3(256), 0, s, (const float*)src, M, C,
                           T_out, src_T, src_off, out);
    return hipGetLastError();
}

}  // namespace vp3d
