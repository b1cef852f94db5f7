// Batched causal streaming step: S independent streams ("slots") of one causal dilated
// TemporalModel (reference common/models/TemporalModel.py:79-138 with causal=True) advance
// together, each at its own stream position t[s].
//
// One launch per layer, the layers of the single stream's `launches` form (stream_step.hip:
// expand, the k-conv and 1x1 of each block, shrink).  For every active slot a layer computes
// what stream_gemv computes for one stream:
//
//   tap k reads the slot's input ring at time t_s - (taps-1-k) dil, clamped at 0 (the
//   reference's edge padding of a causal sequence, generators.py:193-198; stream_step.hip:12-15)
//   the expand's newest tap is the slot's new frame, which is also appended to its frame ring
//   y = [relu](sum * scale + shift) [+ residual row of time t_s]      (TemporalModel.py:132-135)
//   stored to the slot's output ring at t_s & (R - 1)
//
// so a layer is a skinny GEMM, S rows x K by K x N, and the weights -- the traffic of a step --
// are read once per 16-row tile instead of once per stream.  A slot with active[s] == 0 stores
// nothing: no ring slot, no pose row; positions are advanced by a trailing launch.
//
// Look-ahead form (StreamBatchParams::n set): the same step for a NON-causal model
// (TemporalModel.py:79-138 with causal=False, causal_shift = 0), seen P = sum of the layers'
// pads frames late.  In arrival time every tap still reads t_s - (taps-1-k) dil clamped at 0;
// what differs from the causal form:
//   the residual is the centre tap of the block's k-conv window (TemporalModel.py:132 with
//   causal_shift = 0): the block input of time max(t_s - pad_b, 0), not the newest row;
//   a slot takes steps by code: 1 consumes its new frame, 2 drains -- a step whose newest frame
//   is the slot's last consumed one, the right half of the reference's (pad, pad) edge padding
//   (generators.py:193-198), got by clamping the expand's raw-frame taps at frame n_s - 1; the
//   frame ring is not appended to;
//   the shrink stores a pose row only once t_s >= P: the pose of frame t_s - P.
// A slot's state is (t_s steps taken, n_s frames consumed): it has drained iff t_s > n_s and has
// emitted max(t_s - P, 0) poses, so look_takes_step below needs no further counters.
//
// Arithmetic: the exact f32 MFMA (v_mfma_f32_16x16x4_f32) for every weight dtype.  Activations
// stay f32; 16-bit weights are widened to f32 in registers, so only the weights are rounded
// (the streams' contract, oracle/stream_ref.py).
//
// Workgroup (bx, by): output channels [16 bx, 16 bx + 16) of slots [16 by, 16 by + 16), 8 waves.
// The 16 input rows are staged in LDS in chunks of 512 k positions (16 rows x 4096 inputs do not
// fit at once); the chunk after the one being multiplied is already on its way in registers.
// K is split across the waves: K-step b (32 consecutive k) belongs to wave b % 8, and within a
// step lane (r, c) holds the 8 weights W[n0 + r][32 b + 8 c + e] (one 16-byte load at 16 bits,
// two at f32), MFMA e = 0..7 taking k-slot c from k = 32 b + 8 c + e.  Each wave's partial 16 x
// 16 tile goes through LDS and is added in wave order.  The order of an output's sum is thus
// fixed by the layer's K alone: it depends neither on S nor on the slot's row, and a row's
// result depends on that row alone, bit for bit.
//
// Workgroups never wait for each other inside a launch (no spins, granules or atomics): the
// kernel boundaries are the only synchronisation between layers.
#include "kernels.h"

namespace vp3d {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxK = 4096;  // as the single stream (stream_step.hip)
constexpr int kWaves = 8;
constexpr int kThreads = 64 * kWaves;
constexpr int kRows = 16;    // slots per workgroup: one MFMA row tile
constexpr int kCols = 16;    // output channels per workgroup
constexpr int kStepK = 32;   // k positions of a K-step (8 MFMAs)
constexpr int kChunk = 512;  // k positions staged in LDS at a time
constexpr int kPitch = kChunk + 4;  // LDS row pitch in floats: 16-byte aligned, rows 4 banks apart
constexpr int kChunkSteps = kChunk / kStepK;
constexpr int kWaveSteps = kChunkSteps / kWaves;  // K-steps of a chunk per wave
constexpr int kRowsPerWave = kRows / kWaves;      // rows a wave stages
static_assert(kChunkSteps % kWaves == 0 && kRows % kWaves == 0, "chunk geometry");
static_assert(kWaves * kRows * kCols <= kRows * kPitch, "the partial tiles reuse the staging buffer");

// the 8 weights of one lane for one K-step, as loaded
template <typename WT>
struct W8 {
    u32x4 v;
    __device__ __forceinline__ void zero() { v = u32x4{0u, 0u, 0u, 0u}; }
    __device__ __forceinline__ void load(const WT* p) { v = *(const u32x4*)p; }
    __device__ __forceinline__ float get(int e) const {
        typedef WT wt8 __attribute__((ext_vector_type(8)));
        return (float)__builtin_bit_cast(wt8, v)[e];
    }
};

template <>
struct W8<float> {
    f32x4 lo, hi;
    __device__ __forceinline__ void zero() { lo = hi = f32x4{0.f, 0.f, 0.f, 0.f}; }
    __device__ __forceinline__ void load(const float* p) {
        lo = *(const f32x4*)p;
        hi = *(const f32x4*)(p + 4);
    }
    __device__ __forceinline__ float get(int e) const { return e < 4 ? lo[e] : hi[e - 4]; }
};

// Look-ahead form: does a slot with step code `code`, t steps taken and n frames consumed take
// this step?  Consume: only while the slot has never drained (t == n).  Drain: only with a
// frame consumed and poses still owed (t - P < n).  Every layer's launch and the trailing
// advance evaluate this on the same (code, t, n), so they agree.
__device__ __forceinline__ bool look_takes_step(int code, int t, int n, int P) {
    if (code == kStreamCodeConsume) return t == n;
    if (code == kStreamCodeDrain) return n > 0 && t - P < n;
    return false;
}

// VEC: cin and every per-slot stride are multiples of 4 floats, so a lane stages 4 consecutive
// k (one tap) with one 16-byte load; otherwise one k per load (the expand: cin = J_in F)
//
// LOOK: the look-ahead form (header comment).  A template flag, so that the causal form's
// instruction stream stays what it was.
template <typename WT, bool VEC, bool LOOK>
__global__ __launch_bounds__(kThreads) void stream_batch_layer(StreamBatchParams q) {
    __shared__ __attribute__((aligned(16))) float x[kRows * kPitch];
    __shared__ int s_t[kRows], s_on[kRows];
    __shared__ int s_hi[LOOK ? kRows : 1];  // LOOK: the newest raw frame the slot's expand may read
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, c = lane >> 4;
    const int n0 = blockIdx.x * kCols;
    const int row0 = blockIdx.y * kRows;
    const int nsteps = q.Kp / kStepK;
    const int nchunks = (q.Kp + kChunk - 1) / kChunk;

    if (tid < kRows) {
        const int s = row0 + tid;
        if constexpr (LOOK) {
            const int code = s < q.S ? q.active[s] : kStreamCodeIdle;
            const int t = s < q.S ? q.t[s] : 0, n = s < q.S ? q.n[s] : 0;
            const bool on = look_takes_step(code, t, n, q.lookahead);
            s_on[tid] = on ? 1 : 0;
            s_t[tid] = on ? t : 0;
            // a consuming slot's newest frame is the new one (time t == n); a draining slot
            // repeats frame n - 1, the reference's right edge padding
            s_hi[tid] = on ? (code == kStreamCodeConsume ? t : n - 1) : 0;
        } else {
            const bool on = s < q.S && q.active[s] != 0;
            s_on[tid] = on ? 1 : 0;
            s_t[tid] = on ? q.t[s] : 0;
        }
    }

    // the weights do not depend on the positions: the first chunk's loads go out before them
    const WT* const wrow = (const WT*)q.W + (int64_t)(n0 + r) * q.Kp + 8 * c;
    W8<WT> w[kWaveSteps];
    auto load_w = [&](int chunk) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < kWaveSteps; ++j) {
            const int b = chunk * kChunkSteps + j * kWaves + wid;
            if (b < nsteps) w[j].load(wrow + (int64_t)b * kStepK);
        }
    };
#pragma unroll
    for (int j = 0; j < kWaveSteps; ++j) w[j].zero();
    load_w(0);
    __syncthreads();

    // source row of tap time t_s - back for staged row `row` (stream_step.hip's rule)
    auto src_of = [&](int row, int back) __attribute__((always_inline)) -> const float* {
        const int t = s_t[row];
        int tt = t - back;
        tt = tt < 0 ? 0 : tt;
        if constexpr (LOOK) {
            if (q.in_clamp) tt = tt > s_hi[row] ? s_hi[row] : tt;
        }
        const int64_t s = row0 + row;
        if (q.in_frame && tt == t) return q.in_frame + s * q.cin;
        return q.in + s * q.in_stride + (q.in_R ? (int64_t)(tt & (q.in_R - 1)) * q.cin : 0);
    };

    // the expand layer also appends each active slot's new frame to its frame ring (slot of
    // time t; this step's ring taps read older slots, so no workgroup races with it)
    if (q.in_ring_w && blockIdx.x == 0) {
        for (int row = wid; row < kRows; row += kWaves) {
            if (!s_on[row]) continue;
            if constexpr (LOOK) {
                if (s_hi[row] != s_t[row]) continue;  // a draining slot has no new frame
            }
            const int64_t s = row0 + row;
            float* dst = q.in_ring_w + s * q.in_stride + (int64_t)(s_t[row] & (q.in_R - 1)) * q.cin;
            for (int ch = lane; ch < q.cin; ch += 64) dst[ch] = q.in_frame[s * q.cin + ch];
        }
    }

    // a chunk's input values in flight: wave `wid` stages rows wid, wid + 8; zeros past K, for
    // a slot that is inactive and for a row past S
    constexpr int kVals = VEC ? kChunk / 256 : kChunk / 64;
    f32x4 sv[VEC ? kVals * kRowsPerWave : 1];
    float ss[VEC ? 1 : kVals * kRowsPerWave];
    auto fetch = [&](int chunk) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < kVals; ++j) {
            const int k = chunk * kChunk + (VEC ? 4 * lane + 256 * j : lane + 64 * j);
            const int tap = k / q.cin, ch = k - tap * q.cin;
            const int back = (q.taps - 1 - tap) * q.dil;
#pragma unroll
            for (int i = 0; i < kRowsPerWave; ++i) {
                const int row = wid + i * kWaves;
                const bool in = k < q.K && s_on[row];
                if constexpr (VEC) {
                    sv[j * kRowsPerWave + i] = in ? *(const f32x4*)(src_of(row, back) + ch) : f32x4{0.f, 0.f, 0.f, 0.f};
                } else {
                    ss[j * kRowsPerWave + i] = in ? src_of(row, back)[ch] : 0.f;
                }
            }
        }
    };
    auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < kVals; ++j)
#pragma unroll
            for (int i = 0; i < kRowsPerWave; ++i) {
                float* dst = x + (wid + i * kWaves) * kPitch;
                if constexpr (VEC) {
                    *(f32x4*)(dst + 4 * lane + 256 * j) = sv[j * kRowsPerWave + i];
                } else {
                    dst[lane + 64 * j] = ss[j * kRowsPerWave + i];
                }
            }
    };

    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        if (chunk) __syncthreads();  // every wave has read the previous chunk
        stage();
        __syncthreads();
        W8<WT> wc[kWaveSteps];
#pragma unroll
        for (int j = 0; j < kWaveSteps; ++j) wc[j] = w[j];
        if (chunk + 1 < nchunks) {
            load_w(chunk + 1);
            fetch(chunk + 1);
        }
#pragma unroll
        for (int j = 0; j < kWaveSteps; ++j) {
            const int bl = j * kWaves + wid;  // wave-uniform
            if (chunk * kChunkSteps + bl < nsteps) {
                const float* a = x + r * kPitch + bl * kStepK + 8 * c;
                const f32x4 a0 = *(const f32x4*)a, a1 = *(const f32x4*)(a + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], wc[j].get(e), acc, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], wc[j].get(4 + e), acc, 0, 0, 0);
            }
        }
    }

    // the waves' partial tiles (accumulator layout: column r, rows 4 c + e), added in wave order
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) x[wid * (kRows * kCols) + (4 * c + e) * kCols + r] = acc[e];
    __syncthreads();
    if (tid < kRows * kCols) {
        const int row = tid >> 4, n = n0 + (tid & 15);
        float s = x[tid];
#pragma unroll
        for (int v = 1; v < kWaves; ++v) s += x[v * (kRows * kCols) + tid];
        if (n < q.N && s_on[row]) {
            const int t = s_t[row];
            const int64_t slot = row0 + row;
            float y = s * q.scale[n] + q.shift[n];
            if (q.relu) y = y > 0.f ? y : 0.f;
            int tr = t;  // time of the residual row: the centre tap of the block's k-conv window
            bool store = true;
            if constexpr (LOOK) {
                tr = t - q.res_back;
                tr = tr < 0 ? 0 : tr;
                store = t >= q.out_gate;
            }
            if (q.res) y += q.res[slot * q.res_stride + (int64_t)(q.res_R ? (tr & (q.res_R - 1)) : 0) * q.N + n];
            if (store) q.out[slot * q.out_stride + (int64_t)(q.out_R ? (t & (q.out_R - 1)) : 0) * q.N + n] = y;
        }
    }
}

__global__ __launch_bounds__(64) void stream_batch_advance(int* t, const int* active, int S) {
    const int s = threadIdx.x;
    if (s < S && active[s] != 0) t[s] += 1;
}

__global__ __launch_bounds__(64) void stream_batch_advance_look(int* t, int* n, const int* codes, int* pose_frame,
                                                               int P, int S) {
    const int s = threadIdx.x;
    if (s >= S) return;
    const int code = codes[s], ts = t[s], ns = n[s];
    const bool on = look_takes_step(code, ts, ns, P);
    pose_frame[s] = on && ts >= P ? ts - P : -1;
    if (on) {
        t[s] = ts + 1;
        if (code == kStreamCodeConsume) n[s] = ns + 1;
    }
}

template <typename WT, bool LOOK>
void launch_layer(const StreamBatchParams& q, bool vec, dim3 grid, hipStream_t s) {
    if (vec)
        hipLaunchKernelGGL((stream_batch_layer<WT, true, LOOK>), grid, dim3(kThreads), 0, s, q);
    else
        hipLaunchKernelGGL((stream_batch_layer<WT, false, LOOK>), grid, dim3(kThreads), 0, s, q);
}

template <bool LOOK>
void launch_form(const StreamBatchParams& q, Act wtype, bool vec, dim3 grid, hipStream_t s) {
    if (wtype == Act::F32)
        launch_layer<float, LOOK>(q, vec, grid, s);
    else if (wtype == Act::F16)
        launch_layer<_Float16, LOOK>(q, vec, grid, s);
    else
        launch_layer<__bf16, LOOK>(q, vec, grid, s);
}

}  // namespace

hipError_t launch_stream_batch(const StreamBatchParams& q, Act wtype, hipStream_t s) {
    if (q.Kp > kMaxK || q.Kp % kStepK != 0 || q.K > q.Kp || q.S < 1 || q.S > kStreamBatchMax || q.N < 1 ||
        q.cin < 1)
        return hipErrorInvalidValue;
    if (q.in_ring_w && (!q.in_frame || q.in_R < 1)) return hipErrorInvalidValue;
    const bool vec = ((q.cin | (int)q.in_stride) & 3) == 0 && ((uintptr_t)q.in & 15) == 0 &&
                     ((uintptr_t)q.in_frame & 15) == 0;
    const dim3 grid((q.N + kCols - 1) / kCols, (q.S + kRows - 1) / kRows);
    if (q.n) {
        if (q.lookahead < 0 || q.res_back < 0 || q.out_gate < 0) return hipErrorInvalidValue;
        launch_form<true>(q, wtype, vec, grid, s);
    } else {
        if (q.lookahead || q.res_back || q.in_clamp || q.out_gate) return hipErrorInvalidValue;
        launch_form<false>(q, wtype, vec, grid, s);
    }
    return hipGetLastError();
}

hipError_t launch_stream_batch_advance(int* t, const int* active, int S, hipStream_t s) {
    if (S < 1 || S > kStreamBatchMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_batch_advance, dim3(1), dim3(64), 0, s, t, active, S);
    return hipGetLastError();
}

hipError_t launch_stream_batch_advance_look(int* t, int* n, const int* codes, int* pose_frame, int lookahead, int S,
                                            hipStream_t s) {
    if (S < 1 || S > kStreamBatchMax || lookahead < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_batch_advance_look, dim3(1), dim3(64), 0, s, t, n, codes, pose_frame, lookahead, S);
    return hipGetLastError();
}

}  // namespace vp3d
