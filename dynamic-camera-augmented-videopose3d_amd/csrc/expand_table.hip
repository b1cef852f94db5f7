// The expand table's two small kernels (vp3d_capi.cpp, forward_impl's table path).
//
// The expand conv's output row is a function of (sequence, frame position) alone, so an f16x3
// forward of many windows over few resident frames computes it once per frame into a table --
// row j of sequence i = the expand output for unclamped frames lo + j - lead .. + taps - 1,
// T_tab rows per sequence -- and the block-1 convs read window b's row t at table row
// base[b] + t * s0 (s0 = the expand conv's frame stride).  The table spans the starts
// lo = -(span + ...) .. len - 1 + lead + span (span = the rows a window steps over): a window
// starting before `lo` has only rows whose frames all clamp to frame 0, as the window starting
// at `lo` has, and one starting past len - 1 + lead only rows of the last frame, as the window
// starting there -- so clamping the start into that range reproduces the per-frame edge clamp
// (generators.py:92-100) for every start.
//   window_bases        base[b] = seq_b * T_tab + clamp(start_b) - lo; a sequence outside the
//                       pool is a fault.  With frame tables (vp3d_capi.cpp, plan_frame_tables:
//                       blocks 1 .. d computed once per table row too, level l with its own
//                       pitch) the bases are those of the deepest level: the same clamp, the
//                       pitch of that level in place of T_tab, read at j * step_{d+1}.
//                       Trimmed layout (WindowRegions, vp3d_capi.cpp plan_table_layout): the main
//                       region holds the starts 0 .. max_len - 1 only (a start past a short
//                       sequence's end but below max_len clamps to len - 1 + lead and is served by
//                       it); a clamped start below 0 or from max_len on gets its base in the
//                       sequence's low / high edge segment, and the kernel raises the gate word
//                       to this forward's serial so that the edge launches (which return at
//                       entry otherwise, leaving stale rows nothing reads) fill those segments.
//                       Either layout: the two host-mapped hint words take the serial of the
//                       last launch and of the last launch that met such a start.  Launched at
//                       the front of the forward: the bases' place is written by no table launch
//   gather_table_rows  the windows' rows copied out of the table into the contiguous
//                       (B, T_out) layout the expand conv itself writes (kernel forms without
//                       indirect windows; the bit-identity reference of the tests)
//   replicate_edge_rows the clamp-constant edge rows of a frame table level (vp3d_capi.cpp,
//                       plan_table_edges): the level's convs computed rows a .. b of every
//                       sequence only; rows below a are copies of row a (every frame clamps to
//                       frame 0), rows above b of row b (every frame clamps to the last one)
#include "kernels.h"

namespace vp3d {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void window_bases_kernel(const int32_t* __restrict__ pairs,
                                                           const int32_t* __restrict__ seq_len, int B, int n_seq,
                                                           WindowRegions wr, int lo, int lead,
                                                           int32_t* __restrict__ base, unsigned* fault) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    // (host-mapped: the host reads it without waiting, to choose the next forward's layout)
    if (b == 0 && wr.hint) __hip_atomic_store(wr.hint, wr.serial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (b >= B) return;
    const int2 pr = *(const int2*)(pairs + 2 * b);
    // a sequence outside the pool has no table rows: fault, and a base inside the table so that
    // the convs read valid rows
    const bool ok = pr.x >= 0 && pr.x < n_seq;
    const int hi = seq_len[ok ? pr.x : 0] - 1 + lead;  // (>= lo: lo <= 0, len >= 1, lead >= 0)
    const int st = pr.y < lo ? lo : (pr.y > hi ? hi : pr.y);
    // the region: the main rows, or in the trimmed layout the sequence's low / high edge segment
    const bool low = st < 0, high = st >= wr.max_len;
    int row = pr.x * wr.pitch + (st - wr.main_lo);
    if (wr.epitch > 0 && low) row = wr.edge_row0 + 2 * pr.x * wr.epitch + (st - lo);
    if (wr.epitch > 0 && high) row = wr.edge_row0 + (2 * pr.x + 1) * wr.epitch + (st - wr.max_len);
    base[b] = ok ? row : 0;
    if (!ok && fault) __hip_atomic_fetch_or(fault, kFaultWindowStart, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // a start outside the main region's: opens this forward's edge launches (the serial only
    // grows, so nothing is zeroed per forward), one lane per wave
    const bool edge = ok && (low || high);
    const unsigned long long em = __ballot(edge);
    if (edge && (threadIdx.x & 63) == __ffsll((long long)em) - 1) {
        if (wr.gate) __hip_atomic_fetch_max(wr.gate, wr.serial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (wr.hint) __hip_atomic_store(wr.hint + 1, wr.serial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// out row (b, t) = table row base[b] + t * s0; rows of `row16` 16-byte words, one word per lane,
// kRowsPerWg rows per workgroup trip
template <bool NT>
__global__ __launch_bounds__(256) void gather_table_rows_kernel(const u32x4* __restrict__ table,
                                                                const int32_t* __restrict__ base, int64_t rows,
                                                                int T_out, int s0, int row16, u32x4* __restrict__ out) {
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int b = (int)(r / T_out);
        const int t = (int)(r - (int64_t)b * T_out);
        const u32x4* src = table + (int64_t)(base[b] + t * s0) * row16;
        u32x4* dst = out + r * row16;
        for (int c = threadIdx.x; c < row16; c += 256) {
            const u32x4 v = src[c];
            if (NT)
                __builtin_nontemporal_store(v, dst + c);
            else
                dst[c] = v;
        }
    }
}

// replica r of a sequence (a + pitch - 1 - b of them): row r < a takes row a, row b + 1 + (r - a)
// takes row b; one replica row per workgroup trip, one 16-byte word per lane
__global__ __launch_bounds__(256) void replicate_edge_rows_kernel(u32x4* __restrict__ table, int64_t reps, int per_seq,
                                                                  int pitch, int a, int b, int row16) {
    for (int64_t r = blockIdx.x; r < reps; r += gridDim.x) {
        const int i = (int)(r / per_seq);
        const int j = (int)(r - (int64_t)i * per_seq);
        const int dst_row = j < a ? j : b + 1 + (j - a);
        const int src_row = j < a ? a : b;
        u32x4* const seq = table + (int64_t)i * pitch * row16;
        const u32x4* src = seq + (int64_t)src_row * row16;
        u32x4* dst = seq + (int64_t)dst_row * row16;
        for (int c = threadIdx.x; c < row16; c += 256) dst[c] = src[c];
    }
}

}  // namespace

hipError_t launch_replicate_edge_rows(void* table, int n_seq, int pitch, int a, int b, int row_bytes, hipStream_t s) {
    if (row_bytes % 16 != 0 || row_bytes <= 0 || n_seq <= 0 || a < 0 || b < a || b >= pitch) return hipErrorInvalidValue;
    const int per_seq = a + (pitch - 1 - b);
    if (per_seq == 0) return hipSuccess;
    const int64_t reps = (int64_t)n_seq * per_seq;
    const unsigned grid = (unsigned)(reps < (1 << 20) ? reps : (1 << 20));
    hipLaunchKernelGGL(replicate_edge_rows_kernel, dim3(grid), dim3(256), 0, s, (u32x4*)table, reps, per_seq, pitch, a, b,
                       row_bytes / 16);
    return hipGetLastError();
}

hipError_t launch_window_bases(const int32_t* pairs, const int32_t* seq_len, int B, int n_seq, const WindowRegions& wr,
                               int lo, int lead, int32_t* base, unsigned* fault, hipStream_t s) {
    if (lo > 0 || lead < 0 || wr.main_lo > 0 || wr.main_lo < lo || wr.epitch < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_bases_kernel, dim3((B + 255) / 256), dim3(256), 0, s, pairs, seq_len, B, n_seq, wr, lo,
                       lead, base, fault);
    return hipGetLastError();
}

hipError_t launch_gather_table_rows(const void* table, const int32_t* base, int B, int T_out, int s0,
                                    int row_bytes, void* out, hipStream_t s) {
    if (row_bytes % 16 != 0 || B <= 0 || T_out <= 0) return hipErrorInvalidValue;
    const int64_t rows = (int64_t)B * T_out;
    // nontemporal above the 256 MB Infinity Cache, as the expand conv's own stores (expand_gemm.hip)
    const bool nt = rows * row_bytes > (int64_t)256 << 20;
    const unsigned grid = (unsigned)(rows < (1 << 20) ? rows : (1 << 20));
    if (nt)
        hipLaunchKernelGGL(gather_table_rows_kernel<true>, dim3(grid), dim3(256), 0, s, (const u32x4*)table, base, rows,
                           T_out, s0, row_bytes / 16, (u32x4*)out);
    else
        hipLaunchKernelGGL(gather_table_rows_kernel<false>, dim3(grid), dim3(256), 0, s, (const u32x4*)table, base, rows,
                           T_out, s0, row_bytes / 16, (u32x4*)out);
    return hipGetLastError();
}

}  // namespace vp3d
