// C-ABI of the MI355X-native temporal lifter (declared in include/vp3d.h).
//
// Host-side responsibilities, each mirroring a piece of the reference:
//   * configuration and shape rules  — TemporalModel.py:15-33, 85-124, 152-186
//     (pad / causal_shift / dilation bookkeeping, receptive_field :40-47,
//      total_causal_shift :49-60 incl. quirk Q5)
//   * weight folding and packing     — eval BatchNorm1d (TemporalModel.py:32,117,119)
//     folded to per-channel scale/shift exactly as ATen's CPU batch_norm does
//     (alpha = weight * 1/sqrt(var + eps), beta = bias - mean * alpha); conv
//     weights (Cout, Cin, k) packed tap-major [Cout][k*Cin] for the GEMM kernels
//   * forward orchestration          — TemporalModel._forward_blocks :126-138 and
//     TemporalModelOptimized1f._forward_blocks :188-198, one GEMM launch per conv
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vp3d.h"
#include "kernels.h"
#include "host.h"

using namespace vp3d;

namespace vp3d {
namespace host {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

}  // namespace host
}  // namespace vp3d

using namespace vp3d::host;

namespace vp3d {
namespace host {

int validate_cfg(const vp3d_cfg* c) {
    if (!c) return fail(VP3D_ERR_ARG, "cfg is NULL");
    if (c->n_widths < 1 || c->n_widths > VP3D_MAX_BLOCKS)
        return fail(VP3D_ERR_ASSERT, "filter_widths must have 1..8 entries");
    for (int i = 0; i < c->n_widths; ++i)
        if (c->filter_widths[i] <= 0 || c->filter_widths[i] % 2 == 0)
            return fail(VP3D_ERR_ASSERT, "Only odd filter widths are supported");  // TemporalModel.py:21
    if (c->num_joints_in <= 0 || c->in_features <= 0 || c->num_joints_out <= 0 || c->channels <= 0)
        return fail(VP3D_ERR_ASSERT, "joint/feature/channel counts must be positive");
    if (c->variant != VP3D_VARIANT_DILATED && c->variant != VP3D_VARIANT_STRIDED_1F)
        return fail(VP3D_ERR_ARG, "unknown variant");
    if (c->variant == VP3D_VARIANT_STRIDED_1F && c->dense)
        return fail(VP3D_ERR_ARG, "TemporalModelOptimized1f has no dense option");
    if (c->channels % 8 != 0)
        return fail(VP3D_ERR_ARG, "channels must be a multiple of 8 for the MFMA kernels");
    return VP3D_OK;
}

// pad / causal_shift bookkeeping (TemporalModel.py:31,107-111 and :173-177)
void build_geometry(const vp3d_cfg& c, std::vector<int>& pad_out, std::vector<int>& shift_out,
                    std::vector<Layer>& layers_out) {
    struct {
        std::vector<int>& pad;
        std::vector<int>& causal_shift;
        std::vector<Layer>& layers;
    } hh{pad_out, shift_out, layers_out}, *h = &hh;
    const int* fw = c.filter_widths;
    const bool f1 = c.variant == VP3D_VARIANT_STRIDED_1F;
    h->pad.assign(1, fw[0] / 2);
    h->causal_shift.assign(1, c.causal ? fw[0] / 2 : 0);
    const int C = c.channels;
    const int cin0 = c.num_joints_in * c.in_features;

    h->layers.clear();
    Layer ex;
    ex.cin = cin0;
    ex.cout = C;
    ex.taps = fw[0];
    ex.dil = 1;
    ex.stride = f1 ? fw[0] : 1;
    h->layers.push_back(ex);

    int next_dilation = fw[0];
    for (int i = 1; i < c.n_widths; ++i) {
        const int w = fw[i];
        const int pad_i = (w - 1) * next_dilation / 2;
        h->pad.push_back(pad_i);
        if (f1)
            h->causal_shift.push_back(c.causal ? w / 2 : 0);
        else
            h->causal_shift.push_back(c.causal ? (w / 2) * next_dilation : 0);

        Layer kc;
        kc.cin = C;
        kc.cout = C;
        if (f1) {
            kc.taps = w;
            kc.dil = 1;
            kc.stride = w;
        } else if (c.dense) {
            kc.taps = 2 * pad_i + 1;
            kc.dil = 1;
            kc.stride = 1;
        } else {
            kc.taps = w;
            kc.dil = next_dilation;
            kc.stride = 1;
        }
        h->layers.push_back(kc);

        Layer pw;
        pw.cin = C;
        pw.cout = C;
        pw.taps = 1;
        pw.residual = true;
        if (f1) {
            pw.res_stride = w;
            pw.res_off = h->causal_shift.back() + w / 2;  // TemporalModel.py:192
        } else {
            pw.res_stride = 1;
            pw.res_off = pad_i + h->causal_shift.back();  // TemporalModel.py:132
        }
        h->layers.push_back(pw);
        next_dilation *= w;
    }
    Layer sh;
    sh.cin = C;
    sh.cout = c.num_joints_out * 3;
    sh.taps = 1;
    sh.relu = false;
    h->layers.push_back(sh);

    for (Layer& L : h->layers) {
        if (L.dil == 1) {  // taps are adjacent rows: one contiguous K segment
            L.gemm_taps = 1;
            L.Ktap = L.taps * L.cin;
        } else {
            L.gemm_taps = L.taps;
            L.Ktap = L.cin;
        }
        L.K = L.taps * L.cin;
        L.Kp = (L.K + kPadK - 1) / kPadK * kPadK;
        L.Np = (L.cout + kPadN - 1) / kPadN * kPadN;
    }
}

}  // namespace host
}  // namespace vp3d

namespace {

void build_geometry(vp3d_handle* h) { build_geometry(h->cfg, h->pad, h->causal_shift, h->layers); }

void free_layers(vp3d_handle* h) {
    for (Layer& L : h->layers) {
        hipFree(L.w32);
        hipFree(L.wbf);
        hipFree(L.wh);
        hipFree(L.scale);
        hipFree(L.shift);
        hipFree(L.wfbf);
        hipFree(L.wfh);
        hipFree(L.wx3);
        hipFree(L.scale_x3);
        hipFree(L.shift_x3);
        hipFree(L.scale_x3_f32);
        L.shift_x3 = L.scale_x3_f32 = nullptr;
        L.w32 = nullptr;
        L.wbf = L.wh = nullptr;
        L.scale = L.shift = nullptr;
        L.wfbf = L.wfh = nullptr;
        L.wx3 = nullptr;
        L.scale_x3 = nullptr;
    }
}

// The f16x3 path's epilogue vectors of every layer, folded from the host copies upload_weights
// keeps (Layer::sc_host / sh_host / e_x3) and the handle's activation pre-scale
// (vp3d_set_x3_prescale): layer l's stored split rows hold a * 2^p[l], so a producing layer
// undoes its weights' 2^e and its input's 2^p_in and applies its own 2^p_out,
//   scale_x3 = +-scale * 2^(-e - p_in + p_out),  shift_x3 = shift * 2^p_out
// (p_in = 0 for the expand: raw f32 rows; the residual a 1x1 adds is stored at the chain's
// exponent, which is that layer's p_out).  The shrink has p_out = 0: it absorbs the chain's
// inverse and keeps its bias; scale_x3_f32 is the same inverse for its exact-f32 form.  Powers
// of two only: with every exponent zero these are the bits of the unscaled fold.
int fold_x3(vp3d_handle* h) {
    const int nl = (int)h->layers.size();
    for (int li = 0; li < nl; ++li) {
        Layer& L = h->layers[li];
        const bool is_shrink = li == nl - 1;
        const int p_in = li == 0 ? 0 : h->x3_prescale[li - 1];
        const int p_out = is_shrink ? 0 : h->x3_prescale[li];
        // [cout scales | the fault word's device address] (gemm::x3_range_flag; the kernels
        // run with cout % 64 == 0, so the address is 8-byte aligned at index cout).  The
        // shrink (cout = 51): scales padded with zeros to 64 channels (its split GEMM runs
        // 64 columns, the W rows past cout are zero), no range guard (f32 poses out)
        const int tail = is_shrink ? (L.cout + 63) / 64 * 64 : (L.cout + 1) & ~1;
        std::vector<float> scx3(tail + 2, 0.f), shx3(tail, 0.f);
        for (int o = 0; o < L.cout; ++o) {
            scx3[o] = std::ldexp(L.balance_x3 && (o & 1) ? -L.sc_host[o] : L.sc_host[o], -L.e_x3 - p_in + p_out);
            shx3[o] = std::ldexp(L.sh_host[o], p_out);
        }
        static_assert(sizeof(unsigned*) == 2 * sizeof(float), "pointer = two floats");
        std::memcpy(&scx3[tail], &h->sk_err_dev, sizeof(unsigned*));
        if (!L.scale_x3) HIP_TRY(hipMalloc(&L.scale_x3, scx3.size() * 4));
        if (!L.shift_x3) HIP_TRY(hipMalloc(&L.shift_x3, shx3.size() * 4));
        HIP_TRY(hipMemcpy(L.scale_x3, scx3.data(), scx3.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(L.shift_x3, shx3.data(), shx3.size() * 4, hipMemcpyHostToDevice));
        if (is_shrink) {
            std::vector<float> s32(L.cout);
            for (int o = 0; o < L.cout; ++o) s32[o] = std::ldexp(L.sc_host[o], -p_in);
            if (!L.scale_x3_f32) HIP_TRY(hipMalloc(&L.scale_x3_f32, s32.size() * 4));
            HIP_TRY(hipMemcpy(L.scale_x3_f32, s32.data(), s32.size() * 4, hipMemcpyHostToDevice));
        }
    }
    return VP3D_OK;
}

int upload_weights(vp3d_handle* h, const float* const* w, int n) {
    const int expect = vp3d_weight_count(&h->cfg);
    if (!w) return fail(VP3D_ERR_ARG, "weights is NULL");
    if (n != expect)
        return fail(VP3D_ERR_ARG, "expected " + std::to_string(expect) + " weight arrays, got " +
                                      std::to_string(n));
    for (int i = 0; i < n; ++i)
        if (!w[i]) return fail(VP3D_ERR_ARG, "weight array " + std::to_string(i) + " is NULL");
    const float eps = h->cfg.bn_eps;
    const int nl = (int)h->layers.size();
    int wi = 0;
    for (int li = 0; li < nl; ++li) {
        Layer& L = h->layers[li];
        const bool is_shrink = li == nl - 1;
        const float* cw = w[wi++];  // (cout, cin, taps)
        std::vector<float> p32((size_t)L.Np * L.Kp, 0.f);
        for (int o = 0; o < L.cout; ++o)
            for (int c = 0; c < L.cin; ++c)
                for (int k = 0; k < L.taps; ++k)
                    p32[(size_t)o * L.Kp + (size_t)k * L.cin + c] =
                        cw[((size_t)o * L.cin + c) * L.taps + k];
        std::vector<float> sc(L.cout), shv(L.cout);
        if (!is_shrink) {
            const float* g = w[wi++];
            const float* b = w[wi++];
            const float* mu = w[wi++];
            const float* var = w[wi++];
            for (int o = 0; o < L.cout; ++o) {
                const float invstd = 1.0f / std::sqrt(var[o] + eps);
                sc[o] = invstd * g[o];
                shv[o] = b[o] - mu[o] * sc[o];
            }
        } else {
            const float* bias = w[wi++];
            for (int o = 0; o < L.cout; ++o) {
                sc[o] = 1.0f;
                shv[o] = bias[o];
            }
        }
        std::vector<uint16_t> pbf(p32.size()), ph(p32.size());
        for (size_t i = 0; i < p32.size(); ++i) {
            pbf[i] = f32_to_bf16_rne(p32[i]);
            ph[i] = f32_to_f16_rne(p32[i]);
        }
        if (!L.w32) {
            HIP_TRY(hipMalloc(&L.w32, p32.size() * 4));
            HIP_TRY(hipMalloc(&L.wbf, p32.size() * 2));
            HIP_TRY(hipMalloc(&L.wh, p32.size() * 2));
            HIP_TRY(hipMalloc(&L.scale, L.cout * 4));
            HIP_TRY(hipMalloc(&L.shift, L.cout * 4));
        }
        HIP_TRY(hipMemcpy(L.w32, p32.data(), p32.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(L.wbf, pbf.data(), pbf.size() * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(L.wh, ph.data(), ph.size() * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(L.scale, sc.data(), L.cout * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(L.shift, shv.data(), L.cout * 4, hipMemcpyHostToDevice));
        if (li == 0 && !is_shrink && L.K + 2 <= L.Kp) {
            // the expand conv's BN-folded 16-bit copy (expand_gemm.hip)
            std::vector<uint16_t> fbf(p32.size(), 0), fh(p32.size(), 0);
            for (int o = 0; o < L.cout; ++o) {
                for (int k = 0; k < L.K; ++k) {
                    const float v = p32[(size_t)o * L.Kp + k] * sc[o];
                    fbf[(size_t)o * L.Kp + k] = f32_to_bf16_rne(v);
                    fh[(size_t)o * L.Kp + k] = f32_to_f16_rne(v);
                }
                const uint16_t hb = f32_to_bf16_rne(shv[o]), hh = f32_to_f16_rne(shv[o]);
                fbf[(size_t)o * L.Kp + L.K] = hb;
                fh[(size_t)o * L.Kp + L.K] = hh;
                fbf[(size_t)o * L.Kp + L.K + 1] = f32_to_bf16_rne(shv[o] - bf16_to_f32(hb));
                fh[(size_t)o * L.Kp + L.K + 1] = f32_to_f16_rne(shv[o] - f16_to_f32(hh));
            }
            if (!L.wfbf) {
                HIP_TRY(hipMalloc(&L.wfbf, fbf.size() * 2));
                HIP_TRY(hipMalloc(&L.wfh, fh.size() * 2));
            }
            HIP_TRY(hipMemcpy(L.wfbf, fbf.data(), fbf.size() * 2, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(L.wfh, fh.data(), fh.size() * 2, hipMemcpyHostToDevice));
        }
        {
            // split-fp16 copy: W 2^e = hi + lo, both f16 (hi = f16(W 2^e), lo = f16(W 2^e - hi)),
            // the power of two undone exactly by the epilogue scale.
            // Sign-balanced accumulation: odd output channels carry -W and -scale (exact sign
            // flips, the same products).  The f16 MFMA leaves a small offset toward -inf in its
            // f32 accumulator (every channel, whatever the sign of its sum: measured on real
            // block operands through these kernels, tools/ubench/x3_layer_check.hip -- no
            // sign-correlated error, but -1.2..-1.5 x 2^-24 relative once the ReLU keeps the
            // positive outputs only); ReLU turns it into a systematic shrink of the activations
            // (-3.3 x 2^-24 scale at the output of the 5-block stack, tools/x3_depth.py).  On a
            // negated chain the offset lands on +S, so alternating channels cancel it in every
            // layer's output.  VP3D_X3_SIGNS=0 (measurement) keeps every channel positive.
            const char* sg = getenv("VP3D_X3_SIGNS");
            const bool balance = !(sg && strcmp(sg, "0") == 0);
            float wmax = 0.f;
            for (float v : p32) wmax = std::max(wmax, std::fabs(v));
            const int e = wmax > 0.f ? 14 - (int)std::floor(std::log2((double)wmax)) : 0;
            std::vector<uint16_t> px3((size_t)L.Np * 2 * L.Kp, 0);
            for (int o = 0; o < L.cout; ++o)
                for (int k = 0; k < L.Kp; ++k) {
                    const float v = std::ldexp(balance && (o & 1) ? -p32[(size_t)o * L.Kp + k] : p32[(size_t)o * L.Kp + k], e);
                    const uint16_t hi = f32_to_f16_rne(v);
                    const size_t q = (size_t)o * 2 * L.Kp + x3_pos(k);
                    px3[q] = hi;
                    px3[q + 32] = f32_to_f16_rne(v - f16_to_f32(hi));
                }
            if (!L.wx3) HIP_TRY(hipMalloc(&L.wx3, px3.size() * 2));
            HIP_TRY(hipMemcpy(L.wx3, px3.data(), px3.size() * 2, hipMemcpyHostToDevice));
            // the epilogue vectors (scale_x3, shift_x3) are folded from these by fold_x3
            L.sc_host = sc;
            L.sh_host = shv;
            L.e_x3 = e;
            L.balance_x3 = balance;
        }
    }
    return fold_x3(h);
}

// Temporal length after each layer for an input of T frames; returns false if
// T is too short or the residual slice would not line up with the block output
// (the reference raises in that case: a size-mismatched add).
}  // namespace

namespace vp3d {
namespace host {

bool layer_lengths(const vp3d_cfg& cfg, const std::vector<int>& pad, const std::vector<Layer>& layers, int T,
                   std::vector<int>& len) {
    struct {
        const vp3d_cfg& cfg;
        const std::vector<int>& pad;
        const std::vector<Layer>& layers;
    } hh{cfg, pad, layers}, *h = &hh;
    len.clear();
    int L = T;
    for (const Layer& ly : h->layers) {
        const int span = (ly.taps - 1) * ly.dil + 1;
        if (L < span) return false;
        const int out = (L - span) / ly.stride + 1;
        if (ly.residual) {
            // block input length is len[len.size()-2] (input of the k-conv)
        }
        len.push_back(out);
        L = out;
    }
    // residual consistency: block b (1-based) input length = len[2b-2], output len[2b]
    const int nb = h->cfg.n_widths - 1;
    for (int b = 1; b <= nb; ++b) {
        const Layer& pw = h->layers[2 * b];
        const int lin = len[2 * b - 2];
        const int lout = len[2 * b];
        int rlen;
        if (pw.res_stride == 1)
            rlen = lin - 2 * h->pad[b];
        else
            rlen = (lin - pw.res_off + pw.res_stride - 1) / pw.res_stride;
        if (rlen != lout) return false;
    }
    return true;
}

}  // namespace host
}  // namespace vp3d

namespace {

bool layer_lengths(const vp3d_handle* h, int T, std::vector<int>& len) {
    return layer_lengths(h->cfg, h->pad, h->layers, T, len);
}

// bytes per activation element: f32, one 16-bit value, or a split-fp16 (hi, lo) pair
size_t esize(int dtype) { return dtype == VP3D_DTYPE_F32 || dtype == VP3D_DTYPE_F16X3 ? 4 : 2; }

// `first`: the first layer whose output lives in the rotating buffers (1 when the expand conv
// writes the expand table instead, forward_impl's table path)
int ensure_ws(vp3d_handle* h, int B, int T, int dtype, int first = 0) {
    std::vector<int> len;
    if (!layer_lengths(h, T, len)) return fail(VP3D_ERR_ARG, "input too short for the receptive field");
    const size_t rows = (size_t)B * len[first];
    // three rotating activation buffers + (16-bit path) the packed expand-conv rows
    const size_t need = 3 * rows * h->cfg.channels * esize(dtype) +
                        (dtype == VP3D_DTYPE_F32 ? 0 : rows * h->layers[0].Kp * (dtype == VP3D_DTYPE_F16X3 ? 4 : 2));
    if (need <= h->ws_bytes) return VP3D_OK;
    if (h->ws) HIP_TRY(hipFree(h->ws));
    h->ws = nullptr;
    h->ws_bytes = 0;
    HIP_TRY(hipMalloc(&h->ws, need));
    h->ws_bytes = need;
    return VP3D_OK;
}

// the split-fp16 path runs every conv but the shrink on conv_gemm_q64's X3 mode
bool x3_supported(const vp3d_handle* h) { return h->cfg.channels % 64 == 0 && h->cfg.channels <= 1024; }
const char* x3_requirement() { return "dtype f16x3 needs channels % 64 == 0 and channels <= 1024"; }

// The split-K workspace (kSplitPartBytes of partial sums + the tile flags) and the host-mapped
// fault word, on the first layer whose a4 plan splits (not on every handle)
int ensure_fault_word(vp3d_handle* h) {
    if (h->sk_err_host) return VP3D_OK;
    HIP_TRY(hipHostMalloc((void**)&h->sk_err_host, 4, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer((void**)&h->sk_err_dev, h->sk_err_host, 0));
    *(volatile unsigned*)h->sk_err_host = 0u;
    return VP3D_OK;
}

// the control block (vp3d::SplitCtl: wait bound, fault word, fault injection) into the split
// workspace, staged in the handle (the source of the async copy lives as long as the handle)
int write_split_ctl(vp3d_handle* h, unsigned long long spin, int drop, hipStream_t s) {
    h->sk_ctl_stage = vp3d::SplitCtl{spin, h->sk_err_dev, drop, 0};
    HIP_TRY(hipMemcpyAsync((char*)h->sk_ws + kSplitPartBytes + vp3d::kSplitCtlOffset, &h->sk_ctl_stage,
                           sizeof(vp3d::SplitCtl), hipMemcpyHostToDevice, s));
    h->sk_ctl_spin = spin;
    h->sk_ctl_drop = drop;
    return VP3D_OK;
}

int ensure_split_ws(vp3d_handle* h, hipStream_t s) {
    if (h->sk_ws) return VP3D_OK;
    if (const int rc = ensure_fault_word(h)) return rc;
    void* ws = nullptr;
    HIP_TRY(hipMalloc(&ws, vp3d::kSplitPartBytes + vp3d::kSplitFlagBytes));
    const hipError_t e = hipMemsetAsync((char*)ws + vp3d::kSplitPartBytes, 0, vp3d::kSplitFlagBytes, s);
    if (e != hipSuccess) {
        hipFree(ws);
        return fail(VP3D_ERR_HIP, std::string("split-K flags: ") + hipGetErrorString(e));
    }
    h->sk_ws = ws;
    // the production control block, written once with the workspace (no synchronisation)
    return write_split_ctl(h, vp3d::kSplitSpinTicks, 0, s);
}

// the workspace into p when a4 would split this layer (allocated then), else none; the
// control block follows VP3D_A4_SPLIT_SPIN_TICKS / VP3D_A4_SPLIT_DROP (fault-injection tests)
int attach_split_ws(vp3d_handle* h, ConvGemmParams& p, hipStream_t s) {
    if (!conv_gemm_a4_would_split(p)) return VP3D_OK;
    const int rc = ensure_split_ws(h, s);
    if (rc) return rc;
    const char* sp = getenv("VP3D_A4_SPLIT_SPIN_TICKS");
    const char* dr = getenv("VP3D_A4_SPLIT_DROP");
    const unsigned long long spin = sp ? strtoull(sp, nullptr, 10) : vp3d::kSplitSpinTicks;
    const int drop = dr && atoi(dr) != 0 ? 1 : 0;
    if (spin != h->sk_ctl_spin || drop != h->sk_ctl_drop) {
        // tests only: the staging copy may still be the source of the previous async copy
        HIP_TRY(hipStreamSynchronize(s));
        if (const int rc2 = write_split_ctl(h, spin, drop, s)) return rc2;
    }
    p.sk_part = (float*)h->sk_ws;
    p.sk_flag = (int*)((char*)h->sk_ws + kSplitPartBytes);
    return VP3D_OK;
}

// the f16x3 forward's shrink on the split-fp16 tail kernels (default since round 6) or, with
// VP3D_X3_SHRINK=f32 (measurement; read at every forward), the exact f32 GEMM over f32 rows
bool x3_split_shrink(const vp3d_handle* h) {
    const char* e = getenv("VP3D_X3_SHRINK");
    return !(e && strcmp(e, "f32") == 0) && h->layers.back().cout <= 64;  // (one 64-column block)
}

constexpr const char* kSplitFaultMsg =
    "split-K: an owner tile timed out waiting for its helper units (an earlier forward on this "
    "handle produced wrong poses); vp3d_sync_status clears the fault";
constexpr const char* kNonFiniteMsg =
    "f16x3: an earlier forward on this handle split an activation past the f16 range (|x| <= "
    "65504) or produced non-finite poses; its outputs are not valid -- run those inputs in fp32 "
    "(with an activation pre-scale set: re-calibrate with more headroom or clear the pre-scale). "
    "vp3d_sync_status clears the fault";
constexpr const char* kWindowStartMsg =
    "f16x3 expand table: an earlier forward on this handle had a window that names a sequence outside "
    "the pool, [0, n_seq); its outputs are not valid. vp3d_sync_status clears the fault";
const char* fault_msg(unsigned w) {
    if (w & vp3d::kFaultSplitTimeout) return kSplitFaultMsg;
    return (w & vp3d::kFaultWindowStart) && !(w & vp3d::kFaultNonFinite) ? kWindowStartMsg : kNonFiniteMsg;
}

// The expand table (expand_table.hip): whether an f16x3 gathered forward computes the expand conv
// once per resident frame, and how block 1 reads it.  Decided from sizes (and VP3D_EXPAND_TABLE,
// read here once per forward) alone.
struct TablePlan {
    int mode = 0;   // 0: the expand conv per window row; 1: block 1 reads the table through
                    // indirect windows (conv_gemm_a4); 2: the windows' rows copied out of it
    int T_tab = 0;  // table rows per sequence
    int lo = 0;     // the window start table row 0 of a sequence stands for (<= 0, expand_table.hip)
    int s0 = 1;     // table rows between consecutive rows of a window (the expand conv's stride)
    int b_pad = 0;  // int32 slots of the window bases in front of the table
    size_t table_bytes = 0;
    bool forced = false;  // VP3D_EXPAND_TABLE=1 / copy
    // Frame tables (mode 1 only): blocks 1 .. depth are computed once per table row as well, level
    // l = block l's output, one row per frame position.  pitch[l]: rows per sequence of level l
    // (pitch[0] = T_tab; each level loses its k-conv's reach); step[l]: table rows between
    // consecutive rows of a window at level l (step[0] = s0).  Block depth + 1 reads level `depth`
    // through the window bases.
    int depth = 0;
    std::vector<int> pitch, step;
    int max_base = 0;  // the largest row base inside a sequence: clamp(start) - lo <= max_base
    bool ix_allowed = false;  // indirect windows not ruled out (copy on request, VP3D_GEMM=q64, f32 rows)
    // The layout of the rows computed (plan_table_layout; every take-or-refuse decision above is
    // made on the nominal, wide row count).  Wide: one main region per sequence for the starts
    // lo .. max_len - 1 + lead (main_lo = lo, no edge segments).  Trimmed (mode 1 only): the main
    // region serves the starts 0 .. max_len - 1 alone (main_lo = 0; T_tab / pitch[] are then its
    // pitches), and two edge segments per sequence -- the starts lo .. -1 and max_len .. max_len
    // - 1 + lead, `epitch[l]` rows each at level l, from row edge_row0 of every slot on -- are
    // filled by gated launches that run only in a forward whose batch holds such a start.
    bool trimmed = false;
    int main_lo = 0;
    int max_len = 0;
    int edge_row0 = 0;
    std::vector<int> epitch;
    // The main-region rows the convs of level l compute (plan_table_edges): row_a[l] .. row_b[l];
    // the rows outside are copies of those two (0 .. pitch[l] - 1: every row computed).
    std::vector<int> row_a, row_b;
};
// Table rows may number at most 1 / kTableFactor of the window rows they replace: the margin the
// table paths were introduced with, never measured, and kept wherever no measurement covers it --
// a table launch shorter than one round (one round costs the same whatever its fill).  For table
// launches of at least one round (nominal table tiles >= the CUs a4 fills) the measured rule:
// nominal table rows <= kTableRatioNum / kTableRatioDen of the window rows
// (profiles/r09_table_depth_crossover.txt).
constexpr int kTableFactor = 2;
constexpr int kTableRatioNum = 1, kTableRatioDen = 1;
// one rule for the expand table and every frame-table level: `rows` nominal table rows of `C`
// channels against the `wrows` window rows of the block that reads them
bool table_pays(int64_t rows, int64_t wrows, int C) {
    const int round = vp3d::conv_gemm_a4_round_tiles();
    if (round <= 0 || vp3d::conv_gemm_a4_tiles(rows, C) < round) return rows <= wrows / kTableFactor;
    return rows * kTableRatioDen <= wrows * kTableRatioNum;
}

// The f16x3 launch geometry of block layer L (k-conv, or 1x1 + residual) computed once per table
// row: one pseudo-window per sequence at frame stride 1 over the level below -- `pitch_in` rows per
// sequence, consecutive rows of a window `step` table rows apart -- so tap k of output row q reads
// row q + k dil step and the residual slice row q + res_off step.  A plain direct launch: the
// dilated-conv parameters sequence mode runs.
void table_layer_geometry(ConvGemmParams& p, const Layer& L, int n_seq, int pitch_in, int step) {
    const int pitch_out = pitch_in - (L.taps - 1) * L.dil * step;
    p.M = n_seq * pitch_out;
    p.T_out = pitch_out;
    p.T_in = pitch_in;
    p.stride = 1;
    p.dil = L.dil * step;
    p.Ktap = 2 * L.cin;  // every tap its own K segment, the K order unchanged
}
void table_residual_geometry(ConvGemmParams& p, const Layer& L, int pitch_res, int step) {
    p.R_T = pitch_res;
    p.R_stride = 1;
    p.R_off = L.res_off * step;
}
// ... and of block layer L read through the window bases in front of the deepest table (`b_pad`
// int32 slots): window b's input row j is table row base[b] + j step
void indirect_layer_geometry(ConvGemmParams& p, const Layer& L, int b_pad, int step) {
    if (L.residual) {  // the 1x1: its residual slice out of the table
        p.R_T = -b_pad;
        p.R_stride = L.res_stride * step;
        p.R_off = L.res_off * step;
    } else {  // the k-conv: tap k of output row r at base[b] + (r stride + k dil) step
        p.T_in = -b_pad;
        p.stride = L.stride * step;
        p.dil = L.dil * step;
        p.Ktap = 2 * L.cin;
    }
}
// the sizes, pitches and (stand-in) pointers of an f16x3 block layer for the eligibility rules
ConvGemmParams x3_probe(const Layer& L, int M, int T_out, int T_in) {
    void* const al = (void*)(uintptr_t)256;  // (the pointers only stand for their alignment)
    ConvGemmParams q{};
    q.A = q.W = al;
    q.Y = al;
    q.M = M;
    q.N = L.cout;
    q.K = L.K;
    q.Kp = 2 * L.Kp;
    q.T_out = T_out;
    q.T_in = T_in;
    q.stride = L.stride;
    q.dil = L.dil;
    q.Ktap = 2 * L.Ktap;
    q.lda = 2 * L.cin;
    q.ldy = 2 * L.cout;
    q.relu = 1;
    if (L.residual) {
        q.R = al;
        q.ldr = 2 * L.cout;
        q.R_stride = L.res_stride;
        q.R_off = L.res_off;
    }
    return q;
}

// The frame-table depth of a forward whose expand table passed its own rules (tp.mode != 0, indirect
// windows not ruled out): the deepest d <= blocks - 1 (and <= VP3D_FRAME_TABLES, which also lifts
// the size rule) such that at every level 1 .. d the table a block reads passes the size rule
// against that block's window rows (table_pays, on the nominal rows: those of the wide layout,
// whichever layout is then computed) and both its launches run a4's whole / half-N /
// quarter-N tiles (eligible without the split workspace: no split-K plan, no split-K tail, never
// q64), and both layers of block d + 1 take indirect windows; a level whose consumer does not is
// passed over for the next shallower one that does, down to depth 0 = plan_expand_table's own
// choice.  Every table is smaller than level 0's, so the 2 GiB rule holds for all.  Fills
// tp.depth / pitch / step, and makes the plan an indirect one (mode 1) for a depth >= 1.
void plan_frame_tables(const vp3d_handle* h, int B, const std::vector<int>& len, int n_seq, TablePlan& tp) {
    tp.depth = 0;
    tp.pitch.assign(1, tp.T_tab);
    tp.step.assign(1, tp.s0);
    if (tp.mode == 0 || !tp.ix_allowed) return;
    const int nl = (int)h->layers.size();
    int want = (nl - 2) / 2 - 1;  // the last block and the shrink always run per window
    bool force = false;
    if (const char* e = getenv("VP3D_FRAME_TABLES")) {
        want = std::min(want, std::max(0, atoi(e)));
        force = true;
    }
    const int C = h->layers[0].cout;
    int ok_depth = 0;  // the deepest level whose consumer block takes indirect windows
    for (int l = 1; l <= want; ++l) {
        const Layer &Lk = h->layers[2 * l - 1], &Lp = h->layers[2 * l];
        const int pin = tp.pitch[l - 1], st = tp.step[l - 1];
        const int pout = pin - (Lk.taps - 1) * Lk.dil * st;
        if (!Lk.relu || Lk.residual || !Lp.relu || !Lp.residual || Lp.taps != 1 || Lp.stride != 1 ||
            Lp.res_stride != Lk.stride || Lk.cin != C || Lk.cout != C || Lp.cout != C || pout <= 0)
            break;
        // the last row a window reads at this level lies inside its sequence's rows
        if ((int64_t)tp.max_base + (int64_t)(len[2 * l] - 1) * st * Lk.stride >= pout) break;
        if (!force && !table_pays((int64_t)n_seq * pin, (int64_t)B * len[2 * l - 1], C)) break;
        ConvGemmParams q = x3_probe(Lk, 0, 0, 0);
        table_layer_geometry(q, Lk, n_seq, pin, st);
        ConvGemmParams r = x3_probe(Lp, 0, 0, 0);
        table_layer_geometry(r, Lp, n_seq, pout, st);
        table_residual_geometry(r, Lp, pin, st);
        if (!vp3d::conv_gemm_a4_x3_eligible(q, false) || !vp3d::conv_gemm_a4_x3_eligible(r, false)) break;
        tp.pitch.push_back(pout);
        tp.step.push_back(st * Lk.stride);
        // block l + 1 over this level's table (the 1x1 of the last block may write f32 rows for
        // the f32 shrink: not an indirect form)
        const Layer &Nk = h->layers[2 * l + 1], &Np = h->layers[2 * l + 2];
        if (nl - 2 == 2 * l + 2 && !x3_split_shrink(h)) continue;
        ConvGemmParams ck = x3_probe(Nk, B * len[2 * l + 1], len[2 * l + 1], 0);
        indirect_layer_geometry(ck, Nk, tp.b_pad, tp.step[l]);
        ConvGemmParams cp = x3_probe(Np, B * len[2 * l + 2], len[2 * l + 2], len[2 * l + 1]);
        indirect_layer_geometry(cp, Np, tp.b_pad, tp.step[l]);
        // (a4 at any tile count: no other kernel reads a table, and a partial round of whole
        // tiles is little against the block rows the tables above it save)
        if (Nk.relu && !Nk.residual && Np.relu && Np.residual && vp3d::conv_gemm_a4_x3_indirect_ok(ck, true) &&
            vp3d::conv_gemm_a4_x3_indirect_ok(cp, true))
            ok_depth = l;
    }
    tp.depth = ok_depth;
    tp.pitch.resize(ok_depth + 1);
    tp.step.resize(ok_depth + 1);
    // block 1 on the table needs no indirect form of its own: the table path whatever
    // plan_expand_table found for the per-window block 1
    if (ok_depth >= 1) tp.mode = 1;
}

TablePlan plan_expand_table(const vp3d_handle* h, int B, const std::vector<int>& len, int dtype, const GatherSrc* gs,
                            int n_seq, int max_len) {
    TablePlan tp;
    const int nl = (int)h->layers.size();
    if (dtype != VP3D_DTYPE_F16X3 || !gs || gs->cams || n_seq <= 0 || max_len <= 0 || nl < 4) return tp;
    const char* e = getenv("VP3D_EXPAND_TABLE");
    if (e && e[0] == '0') return tp;
    const bool force = e && (strcmp(e, "1") == 0 || strcmp(e, "copy") == 0);
    // a forced frame-table depth >= 1 (plan_frame_tables) needs the level-0 table under it
    const char* fe = getenv("VP3D_FRAME_TABLES");
    const bool force_size = force || (fe && atoi(fe) >= 1);
    const Layer& L0 = h->layers[0];
    const int C = L0.cout;
    tp.s0 = L0.stride;
    // starts lo .. max_len - 1 + lead, then the rows a window steps over (expand_table.hip: every
    // start clamps into that range with the per-frame edge clamp's result)
    if (gs->lead < 0) return tp;
    const int64_t span = (int64_t)(len[0] - 1) * tp.s0;
    tp.lo = -(int)(span + std::max(0, L0.taps - 1 - gs->lead));
    const int64_t t_tab = ((int64_t)max_len - 1 + gs->lead - tp.lo + span + 1 + 15) / 16 * 16;
    const int64_t rows = (int64_t)n_seq * t_tab;
    const int64_t bytes = rows * 2 * C * 2;
    // 32-bit lane offsets from the table start (conv_gemm_a4), some slack for the tiles' rebased
    // resources; one rule for both table modes
    if (bytes >= ((int64_t)1 << 31) - 65536) return tp;
    if (!force_size && !table_pays(rows, (int64_t)B * len[0], C)) return tp;
    tp.T_tab = (int)t_tab;
    tp.main_lo = tp.lo;
    tp.max_len = max_len;
    tp.max_base = max_len - 1 + gs->lead - tp.lo;
    tp.table_bytes = (size_t)bytes;
    tp.b_pad = (B + 63) / 64 * 64;
    tp.mode = 2;
    tp.forced = force;
    if (e && strcmp(e, "copy") == 0) return tp;
    // indirect windows where both block-1 convs run the a4 tile forms that take them (the
    // pointers only stand for their alignment here)
    const char* ge = getenv("VP3D_GEMM");
    if (ge && strcmp(ge, "q64") == 0) return tp;
    if (nl - 2 == 2 && !x3_split_shrink(h)) return tp;  // (the 1x1 would write f32 rows)
    tp.ix_allowed = true;
    const Layer &L1 = h->layers[1], &L2 = h->layers[2];
    ConvGemmParams q = x3_probe(L1, B * len[1], len[1], 0);
    indirect_layer_geometry(q, L1, tp.b_pad, tp.s0);
    if (!L1.relu || L1.residual || !vp3d::conv_gemm_a4_x3_indirect_ok(q)) return tp;
    ConvGemmParams r = x3_probe(L2, B * len[2], len[2], len[1]);
    indirect_layer_geometry(r, L2, tp.b_pad, tp.s0);
    if (!L2.relu || !L2.residual || !vp3d::conv_gemm_a4_x3_indirect_ok(r)) return tp;
    tp.mode = 1;
    return tp;
}

// The layout hint: wide when the most recent forward whose bases kernel has run met a start outside
// 0 .. max_len - 1 (the two host-mapped words of window_bases_kernel, read without waiting: a stale
// value only picks the other correct layout), else trimmed.  VP3D_TABLE_TRIM=0|1 forces either.
bool want_trimmed(const vp3d_handle* h) {
    if (const char* e = getenv("VP3D_TABLE_TRIM")) return atoi(e) != 0;
    if (!h->tab_hint_host) return true;
    const unsigned edges = ((volatile unsigned*)h->tab_hint_host)[1];
    const unsigned seen = ((volatile unsigned*)h->tab_hint_host)[0];
    return !(seen != 0 && edges == seen);
}

// Which rows of the planned tables (indirect windows, mode 1; depth decided) a forward computes.
// The wide layout of plan_expand_table spends 368 of 2,656 rows per sequence and level (max_len
// 2,048, lead 121) on starts before frame 0 or past the last frame, which no generator makes.  The
// trimmed layout computes the main region of the starts 0 .. max_len - 1 -- self-contained at every
// level: level l main rows read level l - 1 main rows only -- and keeps the other starts exact
// through the gated edge segments (TablePlan), each of which recomputes the main rows it overlaps
// so that it is self-contained too.  Falls back to the wide layout wherever a trimmed launch would
// leave the a4 tile forms or the rows pass the 2 GiB of the 32-bit lane offsets.
void plan_table_layout(const vp3d_handle* h, const std::vector<int>& len, const GatherSrc* gs, int n_seq,
                       TablePlan& tp) {
    tp.epitch.assign((size_t)tp.depth + 1, 0);
    if (tp.mode != 1 || !want_trimmed(h)) return;
    const int C = h->layers[0].cout;
    const int64_t span = (int64_t)(len[0] - 1) * tp.s0;
    const int emax = std::max(-tp.lo, gs->lead) - 1;  // the largest start offset inside an edge segment
    if (emax < 0) return;
    const int64_t main0 = ((int64_t)tp.max_len + span + 15) / 16 * 16;
    const int64_t edge0 = ((int64_t)emax + 1 + span + 15) / 16 * 16;
    const int64_t rows = (int64_t)n_seq * (main0 + 2 * edge0);
    if (rows * 2 * C * 2 >= ((int64_t)1 << 31) - 65536) return;
    std::vector<int> pitch{(int)main0}, epitch{(int)edge0};
    for (int l = 1; l <= tp.depth; ++l) {
        const Layer &Lk = h->layers[2 * l - 1], &Lp = h->layers[2 * l];
        const int st = tp.step[l - 1], reach = (Lk.taps - 1) * Lk.dil * st;
        const int pout = pitch[l - 1] - reach, eout = epitch[l - 1] - reach;
        const int64_t rd = (int64_t)(len[2 * l] - 1) * st * Lk.stride;  // rows a window steps over
        if (pout <= 0 || eout <= 0 || tp.max_len - 1 + rd >= pout || emax + rd >= eout) return;
        for (int edge = 0; edge < 2; ++edge) {
            const int ns = edge ? 2 * n_seq : n_seq, pin = edge ? epitch[l - 1] : pitch[l - 1];
            ConvGemmParams q = x3_probe(Lk, 0, 0, 0);
            table_layer_geometry(q, Lk, ns, pin, st);
            ConvGemmParams r = x3_probe(Lp, 0, 0, 0);
            table_layer_geometry(r, Lp, ns, pin - reach, st);
            table_residual_geometry(r, Lp, pin, st);
            if (!vp3d::conv_gemm_a4_x3_eligible(q, false) || !vp3d::conv_gemm_a4_x3_eligible(r, false)) return;
        }
        pitch.push_back(pout);
        epitch.push_back(eout);
    }
    tp.trimmed = true;
    tp.main_lo = 0;
    tp.T_tab = (int)main0;
    tp.max_base = tp.max_len - 1;
    tp.pitch = pitch;
    tp.epitch = epitch;
    tp.edge_row0 = (int)(n_seq * main0);
    tp.table_bytes = (size_t)rows * 2 * C * 2;
}

// Which main-region rows of the frame-table levels 1 .. depth the convs compute (either layout;
// `first` = the start row 0 of the region stands for, tp.main_lo).  Row q of level l is a function
// of the frames first + q - lead .. first + q - lead + S_l, clamped to the sequence (S_l: the frame
// span of a level-l row minus 1: S_0 = taps_0 - 1, S_l = S_{l-1} + (taps_l - 1) dil_l step_{l-1}; 2,
// 8, 26, 80 for the 243-frame model).  Where that span ends at or before frame 0 every frame clamps
// to frame 0, and where it begins at or after frame max_len - 1 >= len_i - 1 every frame clamps to
// the sequence's last one -- in every sequence -- so
//   a_l = the largest q with first + q - lead + S_l <= 0   (0 if none),
//   b_l = the smallest q with first + q - lead >= max_len - 1   (pitch_l - 1 if none),
// rows < a_l equal row a_l and rows > b_l equal row b_l: the level's k-conv computes rows a_l ..
// b_l packed, its 1x1 + residual writes them into the level at the table's pitch
// (ConvGemmParams::Y_T), and launch_replicate_edge_rows fills the rest.  A replica is a copy of a
// row the same instruction chain computed from the same inputs: the same bits.  Level 0 (the
// expand fill) and the gated edge segments keep every row.  VP3D_TABLE_EDGES=0 keeps every row
// everywhere; a level keeps them where the shortened launches would leave the a4 tile forms.
void plan_table_edges(const vp3d_handle* h, const GatherSrc* gs, int n_seq, TablePlan& tp) {
    tp.row_a.assign((size_t)tp.depth + 1, 0);
    tp.row_b.resize((size_t)tp.depth + 1);
    for (int l = 0; l <= tp.depth; ++l) tp.row_b[l] = tp.pitch[l] - 1;
    if (tp.mode != 1 || tp.depth == 0) return;
    if (const char* e = getenv("VP3D_TABLE_EDGES"))
        if (atoi(e) == 0) return;
    const Layer& L0 = h->layers[0];
    int64_t S = (int64_t)(L0.taps - 1) * L0.dil;
    for (int l = 1; l <= tp.depth; ++l) {
        const Layer &Lk = h->layers[2 * l - 1], &Lp = h->layers[2 * l];
        const int st = tp.step[l - 1], pin = tp.pitch[l - 1], pout = tp.pitch[l];
        S += (int64_t)(Lk.taps - 1) * Lk.dil * st;
        const int64_t a64 = (int64_t)gs->lead - tp.main_lo - S;
        const int64_t b64 = (int64_t)tp.max_len - 1 + gs->lead - tp.main_lo;
        const int a = (int)std::min<int64_t>(std::max<int64_t>(a64, 0), pout - 1);
        const int b = (int)std::min<int64_t>(std::max<int64_t>(b64, a), pout - 1);
        if (a == 0 && b == pout - 1) continue;
        const int rows = b - a + 1;
        // the shortened launches: the k-conv's rows packed, the 1x1's out at the table's pitch
        ConvGemmParams q = x3_probe(Lk, 0, 0, 0);
        table_layer_geometry(q, Lk, n_seq, pin, st);
        q.M = n_seq * rows;
        q.T_out = rows;
        ConvGemmParams r = x3_probe(Lp, 0, 0, 0);
        table_layer_geometry(r, Lp, n_seq, rows, st);
        table_residual_geometry(r, Lp, pin, st);
        r.Y_T = pout;
        if (!vp3d::conv_gemm_a4_x3_eligible(q, false) || !vp3d::conv_gemm_a4_x3_eligible(r, false) ||
            !vp3d::conv_gemm_a4_x3_pitched_ok(r))
            continue;
        tp.row_a[l] = a;
        tp.row_b[l] = b;
    }
}

// one table slot: [bases | table]; b_pad % 64 == 0 and whole 16-byte rows keep every slot aligned
size_t table_slot_bytes(const TablePlan& tp) { return (size_t)tp.b_pad * 4 + tp.table_bytes; }

// the table allocation (one slot; with frame tables three, rotating through the levels as block
// input, k-conv output and 1x1 output, each the size of level 0) and the table's own pair list
// -- the pair list holds the pseudo-windows of both layouts, so a change of layout uploads nothing:
// (i, lo) of the wide main region, (i, 0) of the trimmed one, then (i, lo), (i, max_len) of the
// edge segments -- and the gate word (device) and the two hint words (host-mapped) of the bases kernel
int ensure_table(vp3d_handle* h, const TablePlan& tp, int n_seq, hipStream_t s) {
    const bool same_pairs = (int)h->tab_pairs_host.size() == 8 * n_seq &&
                            (n_seq == 0 || (h->tab_pairs_host[1] == tp.lo && h->tab_pairs_host[4 * n_seq + 3] == tp.max_len));
    if (!h->tab_gate) {
        HIP_TRY(hipMalloc((void**)&h->tab_gate, 256));
        HIP_TRY(hipMemsetAsync(h->tab_gate, 0, 256, s));
        HIP_TRY(hipHostMalloc((void**)&h->tab_hint_host, 8, hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void**)&h->tab_hint_dev, h->tab_hint_host, 0));
        ((volatile unsigned*)h->tab_hint_host)[0] = 0u;
        ((volatile unsigned*)h->tab_hint_host)[1] = 0u;
    }
    const size_t need = table_slot_bytes(tp) * (tp.depth > 0 ? 3 : 1);
    if (need > h->tab_bytes) {
        if (h->tab_ws) HIP_TRY(hipFree(h->tab_ws));
        h->tab_ws = nullptr;
        h->tab_bytes = 0;
        HIP_TRY(hipMalloc(&h->tab_ws, need));
        h->tab_bytes = need;
    }
    if (!same_pairs) {
        // (the device synchronised by the free: the host list is no copy's source any more)
        if (h->tab_pairs) HIP_TRY(hipFree(h->tab_pairs));
        h->tab_pairs = nullptr;
        h->tab_pairs_host.assign((size_t)8 * n_seq, 0);
        int32_t* const wide = h->tab_pairs_host.data();
        int32_t *const main = wide + 2 * n_seq, *const edge = wide + 4 * n_seq;
        for (int i = 0; i < n_seq; ++i) {
            wide[2 * i] = main[2 * i] = edge[4 * i] = edge[4 * i + 2] = i;
            wide[2 * i + 1] = edge[4 * i + 1] = tp.lo;
            main[2 * i + 1] = 0;
            edge[4 * i + 3] = tp.max_len;
        }
        HIP_TRY(hipMalloc((void**)&h->tab_pairs, (size_t)8 * n_seq * 4));
        HIP_TRY(hipMemcpyAsync(h->tab_pairs, h->tab_pairs_host.data(), (size_t)8 * n_seq * 4, hipMemcpyHostToDevice, s));
    }
    return VP3D_OK;
}

hipEvent_t get_event(vp3d_handle* h) {
    if (!h->free_events.empty()) {
        hipEvent_t e = h->free_events.back();
        h->free_events.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}

}  // namespace

extern "C" {

int vp3d_abi_version(void) { return VP3D_ABI_VERSION; }

const char* vp3d_last_error(void) { return g_last_error.c_str(); }

int vp3d_weight_count(const vp3d_cfg* cfg) {
    if (validate_cfg(cfg) != VP3D_OK) return -1;
    return 5 + 10 * (cfg->n_widths - 1) + 2;
}

int vp3d_create(const vp3d_cfg* cfg, const float* const* weights, int n_weights, vp3d_handle** out) {
    if (!out) return fail(VP3D_ERR_ARG, "out is NULL");
    *out = nullptr;
    int rc = validate_cfg(cfg);
    if (rc) return rc;
    vp3d_handle* h = new vp3d_handle();
    h->cfg = *cfg;
    if (h->cfg.bn_eps <= 0.f) h->cfg.bn_eps = 1e-5f;
    hipGetDevice(&h->device);
    build_geometry(h);
    h->x3_prescale.assign(h->layers.size() - 1, 0);
    // the device fault word (vp3d_sync_status), host-mapped; before the weights: the f16x3
    // layers keep its address after their scale_x3 vectors
    rc = ensure_fault_word(h);
    if (!rc) rc = upload_weights(h, weights, n_weights);
    if (rc) {
        vp3d_destroy(h);
        return rc;
    }
    h->prof_ms.assign(h->layers.size(), 0.0);
    h->prof_n.assign(h->layers.size(), 0);
    h->prof_flop.assign(h->layers.size(), 0.0);
    *out = h;
    return VP3D_OK;
}

int vp3d_load_weights(vp3d_handle* h, const float* const* weights, int n_weights) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    int dev = 0;
    hipGetDevice(&dev);
    if (dev != h->device) return fail(VP3D_ERR_STATE, "handle belongs to another device");
    return upload_weights(h, weights, n_weights);
}

int vp3d_destroy(vp3d_handle* h) {
    if (!h) return VP3D_OK;
    int prev = 0;
    hipGetDevice(&prev);
    hipSetDevice(h->device);
    free_layers(h);
    if (h->ws) hipFree(h->ws);
    if (h->gather_ws) hipFree(h->gather_ws);
    if (h->tab_ws) hipFree(h->tab_ws);
    if (h->tab_pairs) hipFree(h->tab_pairs);
    if (h->tab_gate) hipFree(h->tab_gate);
    if (h->tab_hint_host) hipHostFree(h->tab_hint_host);
    if (h->sk_ws) hipFree(h->sk_ws);
    if (h->x3_stats) hipFree(h->x3_stats);
    if (h->sk_err_host) hipHostFree(h->sk_err_host);
    for (auto& e : h->pending) {
        hipEventDestroy(e.a);
        hipEventDestroy(e.b);
    }
    for (auto e : h->free_events) hipEventDestroy(e);
    hipSetDevice(prev);
    delete h;
    return VP3D_OK;
}

int vp3d_receptive_field(const vp3d_handle* h) {
    if (!h) return -1;
    int frames = 0;
    for (int p : h->pad) frames += p;
    return 1 + 2 * frames;
}

int vp3d_total_causal_shift(const vp3d_handle* h) {
    // Bit-compatible with TemporalModel.py:49-60, including quirk Q5 (the
    // dilated variant's causal_shift is already dilation-scaled and is scaled again).
    if (!h) return -1;
    int frames = h->causal_shift[0];
    int next_dilation = h->cfg.filter_widths[0];
    for (int i = 1; i < h->cfg.n_widths; ++i) {
        frames += h->causal_shift[i] * next_dilation;
        next_dilation *= h->cfg.filter_widths[i];
    }
    return frames;
}

int vp3d_out_frames(const vp3d_handle* h, int T) {
    if (!h) return -1;
    std::vector<int> len;
    if (!layer_lengths(h, T, len)) return -1;
    return len.back();
}

int vp3d_layer_count(const vp3d_handle* h) { return h ? (int)h->layers.size() : -1; }

int vp3d_reserve(vp3d_handle* h, int B, int T, int dtype) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    if (B <= 0) return fail(VP3D_ERR_ASSERT, "batch must be positive");
    if (dtype < 0 || dtype > VP3D_DTYPE_F16X3) return fail(VP3D_ERR_ARG, "unknown dtype");
    if (dtype == VP3D_DTYPE_F16X3 && !x3_supported(h)) return fail(VP3D_ERR_ARG, x3_requirement());
    return ensure_ws(h, B, T, dtype);
}

// The forward of B windows of T frames.  x: (B, T, J_in*F) f32, or nullptr with `gs`
// describing where the windows are gathered from (vp3d_forward_windows).
// `calib` (fp32 only): per-layer device accumulators of the calibration pass; every conv
// layer's f32 output rows (not the shrink's poses) are reduced into calib[layer] after its launch.
// n_seq / max_len (vp3d_forward_windows_pool): the sequences `gs` may refer to and the longest
// one's length -- what the expand table path (plan_expand_table) is decided and sized from.
static int forward_impl(vp3d_handle* h, const float* x, int B, int T, float* y, int dtype, void* stream,
                        const GatherSrc* gs, vp3d::ActStats* calib = nullptr, int n_seq = 0, int max_len = 0) {
    int dev = 0;
    hipGetDevice(&dev);
    if (dev != h->device) return fail(VP3D_ERR_STATE, "handle belongs to another device");
    // Any T the reference's conv/slice length rules accept is accepted (for
    // Optimized1f that is T == RF in practice); too-short inputs and
    // residual/conv length mismatches fail like torch does (RuntimeError).
    std::vector<int> len;
    if (!layer_lengths(h, T, len))
        return fail(VP3D_ERR_ARG, "input of " + std::to_string(T) +
                                      " frames does not fit the receptive field of " +
                                      std::to_string(vp3d_receptive_field(h)));
    // a fault of an earlier launch on this handle (no synchronisation: the word is host-mapped),
    // pending until vp3d_sync_status reports and clears it.  A split-K timeout refuses every
    // forward (the tile flags need re-zeroing); an f16x3 range / non-finite fault refuses only
    // f16x3 forwards, so the fp32 re-run its message recommends goes through
    if (h->sk_err_host) {
        const unsigned fw = *(volatile unsigned*)h->sk_err_host;
        if ((fw & vp3d::kFaultSplitTimeout) || (fw && dtype == VP3D_DTYPE_F16X3))
            return fail(VP3D_ERR_STATE, fault_msg(fw));
    }
    const bool x3 = dtype == VP3D_DTYPE_F16X3;
    if (x3 && !x3_supported(h)) return fail(VP3D_ERR_ARG, x3_requirement());
    // the expand table path (f16x3, gathered, sizes only); with indirect windows the expand
    // output never exists per window, so the buffers hold block 1's rows at most
    TablePlan tp = plan_expand_table(h, B, len, dtype, gs, n_seq, max_len);
    // frame tables: blocks 1 .. depth once per table row too, block depth + 1 the first per window
    plan_frame_tables(h, B, len, n_seq, tp);
    // the copy form costs more than the expand conv it replaces (it writes the same rows after
    // filling the table): only on request, never as the automatic choice
    if (tp.mode == 2 && !tp.forced) tp = TablePlan{};
    // the rows computed: trimmed to the starts inside the sequences, or today's wide range
    if (tp.mode) plan_table_layout(h, len, gs, n_seq, tp);
    GatherSrc tab_gs, etab_gs;
    ConvGemmParams tab_p{}, etab_p{};
    if (tp.mode) {
        // the table's fill: the expand launch itself over one pseudo-window (i, lo) of T_tab rows
        // at frame stride 1 per sequence
        const Layer& L0 = h->layers[0];
        tab_gs = *gs;
        tab_p.M = n_seq * tp.T_tab;
        tab_p.N = L0.cout;
        tab_p.K = L0.K;
        tab_p.Kp = 2 * L0.Kp;
        tab_p.T_out = tp.T_tab;
        tab_p.T_in = T;
        tab_p.stride = 1;
        tab_p.dil = L0.dil;
        tab_p.Ktap = L0.Ktap;
        tab_p.lda = L0.cin;
        tab_p.relu = L0.relu ? 1 : 0;
        tab_p.ldy = 2 * L0.cout;
        tab_p.W = L0.wx3;
        tab_p.scale = L0.scale_x3;
        tab_p.shift = L0.shift_x3;
        tab_p.Y = (void*)(uintptr_t)256;  // (its alignment: the table is placed below)
        const char* xe = getenv("VP3D_X3_EXPAND");
        if ((xe && strcmp(xe, "pack") == 0) || !expand_gemm_x3_eligible(tab_p, &tab_gs)) tp = TablePlan{};
    }
    // the rows of levels 1 .. depth between their clamp-constant edge rows (after the last place
    // the plan can be dropped)
    if (tp.mode) plan_table_edges(h, gs, n_seq, tp);
    if (gs) {
        h->tab_mode = tp.mode;
        h->tab_depth = tp.depth;
        h->tab_layout = tp.mode ? (tp.trimmed ? 2 : 1) : 0;
        h->tab_rows.clear();
        for (int l = 0; tp.mode && l <= tp.depth; ++l) {
            h->tab_rows.push_back(tp.row_a[l]);
            h->tab_rows.push_back(tp.row_b[l] - tp.row_a[l] + 1);
            h->tab_rows.push_back(tp.pitch[l]);
        }
    }
    const int buf_first = tp.mode == 1 ? 2 * tp.depth + 1 : 0;
    int rc = ensure_ws(h, B, T, dtype, buf_first);
    if (rc) return rc;

    hipStream_t s = (hipStream_t)stream;
    char* table = nullptr;
    if (tp.mode) {
        if ((rc = ensure_table(h, tp, n_seq, s))) return rc;
        table = (char*)h->tab_ws + (size_t)tp.b_pad * 4;
        tab_gs.pairs = h->tab_pairs + (tp.trimmed ? 2 * n_seq : 0);
        tab_p.Y = table;
    }
    // the table slots' tables (level 0 in slot 0; slots 1 and 2 only with frame tables)
    void* tbuf[3] = {table, nullptr, nullptr};
    if (tp.depth > 0)
        for (int i = 1; i < 3; ++i) tbuf[i] = table + i * table_slot_bytes(tp);
    // the edge segments of a trimmed layout: the same place in every slot, after the main rows
    const size_t edge_off = tp.trimmed ? (size_t)tp.edge_row0 * 2 * h->layers[0].cout * 2 : 0;
    unsigned serial = 0;
    int dslot = 0;  // the table slot the deepest level lands in (checked where it is launched)
    if (tp.mode) {
        if (h->tab_serial == 0xffffffffu) {
            // the serial would wrap (the gate's atomic max needs it to grow): start over, once
            // in 2^32 forwards, after what is in flight
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(hipMemsetAsync(h->tab_gate, 0, 256, s));
            ((volatile unsigned*)h->tab_hint_host)[0] = 0u;
            ((volatile unsigned*)h->tab_hint_host)[1] = 0u;
            h->tab_serial = 0;
        }
        serial = ++h->tab_serial;
        if (tp.trimmed) {
            // the edge fill: two pseudo-windows (i, lo), (i, max_len) of epitch[0] rows per sequence
            etab_gs = tab_gs;
            etab_gs.pairs = h->tab_pairs + 4 * n_seq;
            etab_p = tab_p;
            etab_p.M = 2 * n_seq * tp.epitch[0];
            etab_p.T_out = tp.epitch[0];
            etab_p.Y = table + edge_off;
            etab_p.gate = h->tab_gate;
            etab_p.gate_serial = serial;
            if (!expand_gemm_x3_eligible(etab_p, &etab_gs))
                return fail(VP3D_ERR_ASSERT, "the edge fill of a trimmed expand table left the f16x3 expand kernels");
        }
        // The windows' bases, at the front of the forward: in front of the slot the deepest level
        // lands in (the rotation of the layer loop below), which no table launch writes.  The same
        // kernel opens this forward's edge launches and leaves the next forward's layout hint.
        for (int li = 1, cur = 0, blk = -1; li <= 2 * tp.depth; ++li) {
            int out = 0;
            while (out == cur || out == blk) ++out;
            if (li & 1) blk = cur;
            cur = dslot = out;
        }
        vp3d::WindowRegions wr{};
        wr.pitch = tp.pitch[tp.depth];
        wr.main_lo = tp.main_lo;
        wr.max_len = tp.max_len;
        wr.edge_row0 = tp.edge_row0;
        wr.epitch = tp.trimmed ? tp.epitch[tp.depth] : 0;
        wr.serial = serial;
        wr.gate = h->tab_gate;
        wr.hint = h->tab_hint_dev;
        const hipError_t be = launch_window_bases(gs->pairs, gs->seq_len, B, n_seq, wr, tp.lo, gs->lead,
                                                  (int32_t*)tbuf[dslot] - tp.b_pad, h->sk_err_dev, s);
        if (be != hipSuccess) return fail(VP3D_ERR_HIP, std::string("window bases: ") + hipGetErrorString(be));
    }
    const Act act = dtype == VP3D_DTYPE_F32 ? Act::F32 : (dtype == VP3D_DTYPE_BF16 ? Act::BF16 : Act::F16);
    const size_t es = esize(dtype);
    const size_t buf_elems = (size_t)B * len[buf_first] * h->cfg.channels;
    char* base = (char*)h->ws;
    void* buf[3] = {base, base + buf_elems * es, base + 2 * buf_elems * es};

    const int nl = (int)h->layers.size();
    const void* cur_in = x;  // f32 input
    int cur_len = T;
    int xin_buf = -1;        // buffer index holding the current block input
    const void* block_in = nullptr;
    int block_len = 0;
    for (int li = 0; li < nl; ++li) {
        const Layer& L = h->layers[li];
        const bool first = li == 0, last = li == nl - 1;
        ConvGemmParams p{};
        p.A = cur_in;
        p.scale = L.scale;
        // f16x3: the shift at the layer's pre-scale (fold_x3); L.shift stays the other paths'
        p.shift = dtype == VP3D_DTYPE_F16X3 ? L.shift_x3 : L.shift;
        p.M = B * len[li];
        p.N = L.cout;
        p.K = L.K;
        p.Kp = L.Kp;
        p.T_out = len[li];
        p.T_in = cur_len;
        p.stride = L.stride;
        p.dil = L.dil;
        p.Ktap = L.Ktap;
        p.lda = L.cin;
        p.relu = L.relu ? 1 : 0;
        p.ldy = L.cout;
        p.W = dtype == VP3D_DTYPE_F32 ? (const void*)L.w32
                                      : (dtype == VP3D_DTYPE_BF16 ? (const void*)L.wbf : (const void*)L.wh);
        // frame tables: the level (block) this layer builds once per table row, 0 = per window;
        // `ilevel`: the level block tp.depth + 1 reads through the window bases, else -1
        const int tlevel = tp.mode == 1 && li >= 1 && li <= 2 * tp.depth ? (li + 1) / 2 : 0;
        const int ilevel = tp.mode == 1 && (li == 2 * tp.depth + 1 || li == 2 * tp.depth + 2) ? tp.depth : -1;
        int out_buf = -1;
        if (last) {
            p.Y = y;
        } else {
            // pick a buffer (a table slot for a table level) that is neither the current input
            // nor the block input
            void* const* const bufs = tlevel ? tbuf : buf;
            for (int bi = 0; bi < 3; ++bi) {
                if (bufs[bi] == cur_in || bufs[bi] == block_in) continue;
                out_buf = bi;
                break;
            }
            p.Y = bufs[out_buf];
        }
        if (L.residual) {
            p.R = block_in;
            p.R_T = block_len;
            p.R_stride = L.res_stride;
            p.R_off = L.res_off;
            p.ldr = L.cout;
        }
        // a table level computed between its clamp-constant edge rows (plan_table_edges): the main
        // launch's rows per sequence and the first of them, else 0
        int erows = 0, erow0 = 0;
        if (tlevel) {
            // (cur_len / block_len are table pitches here)
            table_layer_geometry(p, L, n_seq, cur_len, tp.step[tlevel - 1]);
            if (L.residual) table_residual_geometry(p, L, block_len, tp.step[tlevel - 1]);
            if (tp.row_a[tlevel] > 0 || tp.row_b[tlevel] < tp.pitch[tlevel] - 1) {
                erow0 = tp.row_a[tlevel];
                erows = tp.row_b[tlevel] - erow0 + 1;
            }
        } else if (first && tp.mode) {
            p.M = tab_p.M;  // (the FLOP of the launch made: the table's fill)
        }
        // algorithmic FLOP of the layer (unpadded K), timed from before any packing
        ProfEvent pe{};
        const bool timed = h->profiling && li < 64 && ((h->prof_mask >> li) & 1);
        if (timed) {
            pe.layer = li;
            pe.a = get_event(h);
            pe.b = get_event(h);
            // (the rows the launch computes)
            pe.flop = 2.0 * (double)(erows ? n_seq * erows : p.M) * (double)p.N * (double)p.K;
            hipEventRecord(pe.a, s);
        }
        Act a_type = first ? Act::F32 : act;
        const Act o_type = last ? Act::F32 : act;
        hipError_t e = hipSuccess;
        bool launched = false;
        if (x3 && last && x3_split_shrink(h)) {
            // shrink (round 6): split fp16 over the split rows the layer before wrote, on the
            // split-K tail kernels (conv_gemm_tail.hip) with a fixed 2 K-slices per output -- the
            // same sums at every batch size -- and f32 poses out
            if ((rc = ensure_split_ws(h, s))) return rc;
            p.W = L.wx3;
            p.Kp = 2 * L.Kp;
            p.lda = 2 * L.cin;
            p.Ktap = 2 * L.Ktap;
            p.scale = L.scale_x3;
            p.sk_part = (float*)h->sk_ws;
            e = launch_conv_gemm_x3_shrink(p, s);
            launched = true;
        } else if (x3 && last) {
            // shrink: the exact f32 GEMM over the f32 rows the layer before wrote (rows at the
            // chain's pre-scale: undone by this form's own scale vector, ones without one)
            p.W = L.w32;
            p.scale = L.scale_x3_f32;
            e = launch_conv_gemm(p, Act::F32, Act::F32, Act::F32, s);
            launched = true;
        } else if (x3 && first && tp.mode) {
            // expand table: the expand conv once per resident frame, the windows' bases, then
            // either nothing more (block 1 reads the table through them) or the windows' rows
            // copied out into the layout the per-window expand writes
            e = launch_expand_gemm_x3(tab_p, &tab_gs, s);
            // (the edge segments' fill: returns at entry unless the bases kernel opened the gate)
            if (e == hipSuccess && tp.trimmed) e = launch_expand_gemm_x3(etab_p, &etab_gs, s);
            if (e == hipSuccess && tp.mode == 2)
                e = launch_gather_table_rows(table, (const int32_t*)h->tab_ws, B, len[0], tp.s0, 2 * L.cout * 2, p.Y, s);
            if (tp.mode == 1) p.Y = table;  // (the next layers' input; out_buf stays free)
            launched = true;
        } else if (x3 && first && nl > 2 && [&] {
                       // VP3D_X3_EXPAND=pack (measurement): the pack + GEMM form instead
                       const char* xe = getenv("VP3D_X3_EXPAND");
                       if (xe && strcmp(xe, "pack") == 0) return false;
                       ConvGemmParams q = p;
                       q.W = L.wx3;
                       q.Kp = 2 * L.Kp;
                       q.ldy = 2 * L.cout;
                       return expand_gemm_x3_eligible(q, gs);
                   }()) {
            // split-fp16 expand: the f32 rows (window gather + camera concat fused) split in
            // registers, BN + ReLU in the epilogue, split output rows (expand_gemm.hip)
            p.W = L.wx3;
            p.Kp = 2 * L.Kp;
            p.scale = L.scale_x3;
            p.ldy = 2 * L.cout;
            e = launch_expand_gemm_x3(p, gs, s);
            launched = true;
        } else if (x3) {
            // split fp16: three 16-bit MFMA products per K group on conv_gemm_q64 (X3 mode)
            if (first) {
                // the expand conv's rows (window gather + camera concat fused) packed as halves
                void* packed = base + 3 * buf_elems * es;
                e = launch_pack_rows_x3(gs ? nullptr : x, gs, p.M, p.T_out, p.T_in, p.stride, L.cin, L.K, L.Kp,
                                        packed, h->sk_err_dev, s);
                if (e != hipSuccess) return fail(VP3D_ERR_HIP, std::string("pack: ") + hipGetErrorString(e));
                p.A = packed;
                p.T_in = p.T_out;
                p.stride = 1;
                p.dil = 1;
                p.lda = 2 * L.Kp;
                p.Ktap = 2 * L.Kp;
            } else {
                p.lda = 2 * L.cin;
                p.Ktap = 2 * L.Ktap;
            }
            // the first per-window block's k-conv over the deepest table: window b's input row j
            // is table row base[b] + j step, so tap k of output row r sits at
            // base[b] + (r stride + k dil) step -- every tap its own K segment, the K order unchanged
            if (ilevel >= 0 && !L.residual) indirect_layer_geometry(p, L, tp.b_pad, tp.step[ilevel]);
            if (tlevel) p.Ktap = 2 * L.cin;
            const bool out_f32 = li == nl - 2 && !x3_split_shrink(h);
            p.Kp = 2 * L.Kp;
            p.W = L.wx3;
            p.scale = L.scale_x3;
            p.ldy = out_f32 ? L.cout : 2 * L.cout;
            if (L.residual) p.ldr = 2 * L.cout;
            // that block's residual slice, out of the table
            if (ilevel >= 0 && L.residual) indirect_layer_geometry(p, L, tp.b_pad, tp.step[ilevel]);
            // the one-wave-per-SIMD kernel where it fills the chip (VP3D_GEMM=q64 forces q64)
            const char* ge = getenv("VP3D_GEMM");
            if (tlevel) {
                // a table row must come from the per-row instruction chain of the window row it
                // replaces: a4's whole / half-N / quarter-N tiles only.  No split workspace is
                // attached, so neither a split-K plan nor the split-K tail is planned (also
                // under VP3D_A4_SPLIT=2), and q64 is never the fallback (plan_frame_tables)
                if (out_f32 || !conv_gemm_a4_x3_eligible(p, false))
                    return fail(VP3D_ERR_ASSERT, "frame table layer " + std::to_string(li) + " left the a4 tile forms");
                // the deepest level lands where the bases were written in front of (dslot above)
                if (li == 2 * tp.depth && p.Y != tbuf[dslot])
                    return fail(VP3D_ERR_ASSERT, "the deepest frame table left the slot its window bases are in front of");
                // between the clamp-constant edge rows: the k-conv reads from row a of every sequence
                // on and writes its rows packed; the 1x1 reads those, takes its residual slice from
                // row a on and writes rows a .. b of the level at the table's pitch
                ConvGemmParams pm = p;
                if (erows) {
                    pm.M = n_seq * erows;
                    pm.T_out = erows;
                    if (!L.residual) {
                        pm.A = (const char*)p.A + (size_t)erow0 * p.lda * 2;
                    } else {
                        pm.T_in = erows;
                        pm.R_off = p.R_off + erow0;
                        pm.Y = (char*)p.Y + (size_t)erow0 * p.ldy * 2;
                        pm.Y_T = tp.pitch[tlevel];
                    }
                    if (!conv_gemm_a4_x3_eligible(pm, false) || (L.residual && !conv_gemm_a4_x3_pitched_ok(pm)))
                        return fail(VP3D_ERR_ASSERT, "frame table layer " + std::to_string(li) + " (between its edge rows) left the a4 tile forms");
                }
                e = launch_conv_gemm_a4_x3(pm, false, s);
                // ... and the rows outside a .. b from rows a and b, before anything reads the level
                if (e == hipSuccess && erows && L.residual)
                    e = launch_replicate_edge_rows(p.Y, n_seq, tp.pitch[tlevel], erow0, erow0 + erows - 1, p.ldy * 2, s);
                if (e == hipSuccess && tp.trimmed) {
                    // the same layer over the edge segments (two pseudo-windows per sequence at
                    // their own pitch, after the main rows of the same slots), gated
                    ConvGemmParams q = p;
                    table_layer_geometry(q, L, 2 * n_seq, tp.epitch[L.residual ? tlevel : tlevel - 1], tp.step[tlevel - 1]);
                    if (L.residual) table_residual_geometry(q, L, tp.epitch[tlevel - 1], tp.step[tlevel - 1]);
                    q.A = (const char*)p.A + edge_off;
                    q.Y = (char*)p.Y + edge_off;
                    if (p.R) q.R = (const char*)p.R + edge_off;
                    q.gate = h->tab_gate;
                    q.gate_serial = serial;
                    if (!conv_gemm_a4_x3_eligible(q, false))
                        return fail(VP3D_ERR_ASSERT, "frame table layer " + std::to_string(li) + " (edge segments) left the a4 tile forms");
                    e = launch_conv_gemm_a4_x3(q, false, s);
                }
            } else if ((rc = attach_split_ws(h, p, s))) {
                return rc;
            } else if (!(ge && strcmp(ge, "q64") == 0) &&
                       (conv_gemm_a4_x3_eligible(p, out_f32) || (ilevel >= 1 && !out_f32))) {
                // (the block over a frame table: a4 at any tile count, plan_frame_tables)
                e = launch_conv_gemm_a4_x3(p, out_f32, s);
            } else {
                if (!conv_gemm_q64_x3_eligible(p, out_f32)) return fail(VP3D_ERR_ARG, x3_requirement());
                e = launch_conv_gemm_q64_x3(p, out_f32, s);
            }
            launched = true;
        }
        // the expand kernel takes the BN-folded weights (Layer::wfbf / wfh)
        const void* wfold = act == Act::BF16 ? (const void*)L.wfbf : (const void*)L.wfh;
        ConvGemmParams pf = p;
        pf.W = wfold;
        if (launched) {
        } else if (first && gs && act != Act::F32 && wfold && expand_gather_eligible(pf, *gs, o_type, act)) {
            // the window gather (+ camera concat) fused into the expand conv's operand loads
            e = launch_expand_gemm_gather(pf, *gs, act, s);
            launched = true;
        } else if (first && gs) {
            // any other first-layer path: gather the windows into the scratch tensor first
            const size_t need = (size_t)B * T * L.cin * sizeof(float);
            if (need > h->gather_bytes) {
                if (h->gather_ws) HIP_TRY(hipFree(h->gather_ws));
                h->gather_ws = nullptr;
                h->gather_bytes = 0;
                HIP_TRY(hipMalloc(&h->gather_ws, need));
                h->gather_bytes = need;
            }
            hipError_t ge = launch_gather_windows(gs->kps, gs->f2, gs->cams, gs->seq_off, gs->seq_len,
                                                  gs->pairs, B, T, gs->lead, 0, h->gather_ws, s);
            if (ge != hipSuccess) return fail(VP3D_ERR_HIP, std::string("gather: ") + hipGetErrorString(ge));
            x = h->gather_ws;
            p.A = x;
        }
        if (launched) {
        } else if (first && act != Act::F32 && wfold && expand_gemm_eligible(pf, o_type, act)) {
            // 16-bit expand conv straight from the f32 input rows (expand_gemm.hip)
            pf.A = p.A;
            e = launch_expand_gemm(pf, act, s);
            launched = true;
        } else if (first && act != Act::F32) {
            // 16-bit path for the shapes expand_gemm does not take (K > 160: filter width 5
            // and wider, or more input joints): pack the f32 input rows of the expand conv
            // into zero-padded 16-bit GEMM rows (one launch) so the conv runs on the
            // tap-aligned kernel
            void* packed = base + 3 * buf_elems * es;
            hipError_t pe = launch_pack_rows((const float*)x, p.M, p.T_out, p.T_in, p.stride, p.lda,
                                             p.K, p.Kp, packed, act == Act::BF16, s);
            if (pe != hipSuccess) return fail(VP3D_ERR_HIP, std::string("pack: ") + hipGetErrorString(pe));
            p.A = packed;
            p.K = p.Kp;
            p.Ktap = p.Kp;
            p.lda = p.Kp;
            p.T_in = p.T_out;
            p.stride = 1;
            p.dil = 1;
            a_type = act;
        }
        if (!launched) {
            if (act != Act::F32 && !first && !last && (rc = attach_split_ws(h, p, s))) return rc;
            e = launch_conv_gemm(p, a_type, o_type, act, s);
        }
        if (e != hipSuccess)
            return fail(VP3D_ERR_HIP, std::string("conv layer ") + std::to_string(li) + ": " +
                                          hipGetErrorString(e));
        if (timed) {
            hipEventRecord(pe.b, s);
            h->pending.push_back(pe);
        }
        if (calib && !last) {
            const hipError_t ce = launch_act_stats((const float*)p.Y, (int64_t)p.M * L.cout, calib + (size_t)li * vp3d::kActStatSlots, s);
            if (ce != hipSuccess) return fail(VP3D_ERR_HIP, std::string("activation statistics: ") + hipGetErrorString(ce));
        }
        // the k-conv of a block reads the block input; remember it for the 1x1's residual
        if (!last && !L.residual && !first) {
            block_in = cur_in;
            block_len = cur_len;
        }
        cur_in = p.Y;
        cur_len = tlevel ? p.T_out : (first && tp.mode == 1 ? tp.T_tab : len[li]);
        (void)xin_buf;
    }
    if (x3) {
        // f16x3 carries every activation as f16 halves: one past |x| < 65,504 turns into inf /
        // NaN downstream -- flagged here (one read of the poses), reported by the next call
        if ((rc = ensure_fault_word(h))) return rc;
        const hipError_t e = launch_nonfinite_check(y, (int64_t)B * len.back() * h->layers.back().cout,
                                                    h->sk_err_dev, vp3d::kFaultNonFinite, s);
        if (e != hipSuccess) return fail(VP3D_ERR_HIP, std::string("finite check: ") + hipGetErrorString(e));
    }
    return VP3D_OK;
}

int vp3d_forward(vp3d_handle* h, const float* x, int B, int T, float* y, int dtype, void* stream) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    if (!x || !y) return fail(VP3D_ERR_ARG, "x / y is NULL");
    if (B <= 0) return fail(VP3D_ERR_ASSERT, "batch must be positive");
    if (dtype < 0 || dtype > VP3D_DTYPE_F16X3) return fail(VP3D_ERR_ARG, "unknown dtype");
    return forward_impl(h, x, B, T, y, dtype, stream, nullptr);
}

int vp3d_forward_windows(vp3d_handle* h, const float* kps, int32_t f2, const float* cams, const int64_t* seq_off,
                         const int32_t* seq_len, const int32_t* pairs, int B, int window, int lead, float* y,
                         int dtype, void* stream) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    if (!kps || !seq_off || !seq_len || !pairs || !y) return fail(VP3D_ERR_ARG, "a device pointer is NULL");
    if (B <= 0) return fail(VP3D_ERR_ASSERT, "batch must be positive");
    if (dtype < 0 || dtype > VP3D_DTYPE_F16X3) return fail(VP3D_ERR_ARG, "unknown dtype");
    // bf16's 8-bit mantissa on the metre-scale K.E channels: 30 mm errors on the config-3
    // windows; the camera-conditioned pipeline takes fp16, f16x3 or fp32
    if (cams && dtype == VP3D_DTYPE_BF16)
        return fail(VP3D_ERR_ARG, "bf16 is refused with the camera concat (use fp16, f16x3 or fp32)");
    const int cin = h->cfg.num_joints_in * h->cfg.in_features;
    if (f2 + (cams ? 12 : 0) != cin)
        return fail(VP3D_ERR_ASSERT, "frame features (" + std::to_string(f2) + (cams ? " + 12" : "") +
                                         ") != num_joints_in * in_features (" + std::to_string(cin) + ")");
    GatherSrc g;
    g.kps = kps;
    g.f2 = f2;
    g.cams = cams;
    g.seq_off = seq_off;
    g.seq_len = seq_len;
    g.pairs = pairs;
    g.lead = lead;
    return forward_impl(h, nullptr, B, window, y, dtype, stream, &g);
}

int vp3d_forward_windows_pool(vp3d_handle* h, const float* kps, int32_t f2, const float* cams, const int64_t* seq_off,
                              const int32_t* seq_len, int32_t n_seq, int32_t max_len, const int32_t* pairs, int B,
                              int window, int lead, float* y, int dtype, void* stream) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    if (!kps || !seq_off || !seq_len || !pairs || !y) return fail(VP3D_ERR_ARG, "a device pointer is NULL");
    if (B <= 0) return fail(VP3D_ERR_ASSERT, "batch must be positive");
    if (n_seq <= 0 || max_len <= 0) return fail(VP3D_ERR_ARG, "n_seq and max_len must be positive");
    if (dtype < 0 || dtype > VP3D_DTYPE_F16X3) return fail(VP3D_ERR_ARG, "unknown dtype");
    if (cams && dtype == VP3D_DTYPE_BF16)
        return fail(VP3D_ERR_ARG, "bf16 is refused with the camera concat (use fp16, f16x3 or fp32)");
    const int cin = h->cfg.num_joints_in * h->cfg.in_features;
    if (f2 + (cams ? 12 : 0) != cin)
        return fail(VP3D_ERR_ASSERT, "frame features (" + std::to_string(f2) + (cams ? " + 12" : "") +
                                         ") != num_joints_in * in_features (" + std::to_string(cin) + ")");
    GatherSrc g;
    g.kps = kps;
    g.f2 = f2;
    g.cams = cams;
    g.seq_off = seq_off;
    g.seq_len = seq_len;
    g.pairs = pairs;
    g.lead = lead;
    return forward_impl(h, nullptr, B, window, y, dtype, stream, &g, nullptr, n_seq, max_len);
}

int vp3d_expand_table_mode(const vp3d_handle* h) { return h ? h->tab_mode : -1; }

int vp3d_frame_table_depth(const vp3d_handle* h) { return h ? h->tab_depth : -1; }

int vp3d_table_layout(const vp3d_handle* h, int* edges) {
    if (!h) return -1;
    // (the hint words are the bases kernel's: exact once the forward has completed)
    if (edges)
        *edges = h->tab_layout != 0 && h->tab_hint_host && ((volatile unsigned*)h->tab_hint_host)[1] == h->tab_serial;
    return h->tab_layout;
}

int vp3d_table_rows(const vp3d_handle* h, int level, int* first_row, int* rows, int* pitch) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    if (level < 0 || (size_t)3 * level + 2 >= h->tab_rows.size())
        return fail(VP3D_ERR_ARG, "the last gathered forward had no table level " + std::to_string(level));
    if (first_row) *first_row = h->tab_rows[3 * level];
    if (rows) *rows = h->tab_rows[3 * level + 1];
    if (pitch) *pitch = h->tab_rows[3 * level + 2];
    return VP3D_OK;
}

void vp3d_table_depth_rule(int* factor, int* ratio_num, int* ratio_den) {
    if (factor) *factor = kTableFactor;
    if (ratio_num) *ratio_num = kTableRatioNum;
    if (ratio_den) *ratio_den = kTableRatioDen;
}

int vp3d_sync_status(vp3d_handle* h, void* stream) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (!h->sk_err_host || !*(volatile unsigned*)h->sk_err_host) return VP3D_OK;
    // every launch of this handle on `stream` is done: re-zero the tile flags (a timed-out
    // owner took back counts that never came) and clear the word, then report
    const unsigned w = *(volatile unsigned*)h->sk_err_host;
    if (h->sk_ws && (w & vp3d::kFaultSplitTimeout)) {
        HIP_TRY(hipMemsetAsync((char*)h->sk_ws + vp3d::kSplitPartBytes, 0, vp3d::kSplitCtlOffset, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    }
    *(volatile unsigned*)h->sk_err_host = 0u;
    return fail(VP3D_ERR_STATE, fault_msg(w));
}

int vp3d_set_x3_prescale(vp3d_handle* h, const int32_t* p, int n) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    if (!p) return fail(VP3D_ERR_ARG, "exponents is NULL");
    const int want = (int)h->layers.size() - 1;
    if (n != want)
        return fail(VP3D_ERR_ARG, "f16x3 pre-scale: expected " + std::to_string(want) +
                                      " exponents (one per conv layer output, none for the shrink), got " +
                                      std::to_string(n));
    for (int l = 0; l < n; ++l)
        if (p[l] < -VP3D_X3_PRESCALE_MAX || p[l] > VP3D_X3_PRESCALE_MAX)
            return fail(VP3D_ERR_ARG, "f16x3 pre-scale: layer " + std::to_string(l) + " has exponent " +
                                          std::to_string(p[l]) + ", past +-" + std::to_string(VP3D_X3_PRESCALE_MAX));
    // residual constraint: a block's output is res + relu(bn(z)) with res the block input, so
    // the expand output (layer 0) and every block's 1x1 output (layers 2, 4, ...) share one exponent
    for (int l = 2; l < n; l += 2)
        if (p[l] != p[0])
            return fail(VP3D_ERR_ARG, "f16x3 pre-scale: layer " + std::to_string(l) + " (a block's 1x1 output) has exponent " +
                                          std::to_string(p[l]) + " but the residual chain (layer 0, the expand output) has " +
                                          std::to_string(p[0]) + "; the layers a residual add joins share one exponent");
    int dev = 0;
    hipGetDevice(&dev);
    if (dev != h->device) return fail(VP3D_ERR_STATE, "handle belongs to another device");
    if (std::equal(p, p + n, h->x3_prescale.begin())) return VP3D_OK;
    // a forward in flight may still read the vectors about to be rewritten
    HIP_TRY(hipDeviceSynchronize());
    const std::vector<int> prev = h->x3_prescale;
    h->x3_prescale.assign(p, p + n);
    const int rc = fold_x3(h);
    if (rc) h->x3_prescale = prev;
    return rc;
}

int vp3d_get_x3_prescale(const vp3d_handle* h, int32_t* p, int n) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    if (!p) return fail(VP3D_ERR_ARG, "exponents is NULL");
    if (n != (int)h->x3_prescale.size())
        return fail(VP3D_ERR_ARG, "f16x3 pre-scale: expected room for " + std::to_string(h->x3_prescale.size()) +
                                      " exponents, got " + std::to_string(n));
    std::copy(h->x3_prescale.begin(), h->x3_prescale.end(), p);
    return VP3D_OK;
}

// The calibration pass: the fp32 forward with every conv layer's output reduced on the device
// (act_stats.hip), then the accumulators read back.  Synchronous.
static int calibrate_impl(vp3d_handle* h, const float* x, int B, int T, vp3d_act_stats* out, void* stream,
                          const GatherSrc* gs) {
    if (!out) return fail(VP3D_ERR_ARG, "stats_out is NULL");
    int dev = 0;
    hipGetDevice(&dev);
    if (dev != h->device) return fail(VP3D_ERR_STATE, "handle belongs to another device");
    std::vector<int> len;
    if (!layer_lengths(h, T, len))
        return fail(VP3D_ERR_ARG, "input of " + std::to_string(T) + " frames does not fit the receptive field of " +
                                      std::to_string(vp3d_receptive_field(h)));
    const int n = (int)h->layers.size() - 1;
    hipStream_t s = (hipStream_t)stream;
    const size_t stat_bytes = (size_t)n * vp3d::kActStatSlots * sizeof(vp3d::ActStats);
    if (!h->x3_stats) HIP_TRY(hipMalloc((void**)&h->x3_stats, stat_bytes));
    HIP_TRY(hipMemsetAsync(h->x3_stats, 0, stat_bytes, s));
    float* y = nullptr;
    HIP_TRY(hipMalloc((void**)&y, (size_t)B * len.back() * h->layers.back().cout * sizeof(float)));
    int rc = forward_impl(h, x, B, T, y, VP3D_DTYPE_F32, stream, gs, h->x3_stats);
    std::vector<vp3d::ActStats> host((size_t)n * vp3d::kActStatSlots);
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(host.data(), h->x3_stats, stat_bytes, hipMemcpyDeviceToHost);
    hipFree(y);
    if (rc) return rc;
    if (e != hipSuccess) return fail(VP3D_ERR_HIP, std::string("calibration read-back: ") + hipGetErrorString(e));
    for (int l = 0; l < n; ++l) {
        const double count = (double)B * len[l] * h->layers[l].cout;
        unsigned bits = 0;
        double sumsq = 0.0;
        unsigned long long small = 0;
        for (int k = 0; k < vp3d::kActStatSlots; ++k) {
            const vp3d::ActStats& t = host[(size_t)l * vp3d::kActStatSlots + k];
            bits = std::max(bits, t.absmax_bits);
            sumsq += t.sumsq;
            small += t.small;
        }
        float amax;
        std::memcpy(&amax, &bits, 4);
        out[l].absmax = (double)amax;
        out[l].rms = std::sqrt(sumsq / count);
        out[l].small_share = (double)small / count;
    }
    return VP3D_OK;
}

int vp3d_x3_calibrate(vp3d_handle* h, const float* x, int B, int T, vp3d_act_stats* stats_out, void* stream) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    if (!x) return fail(VP3D_ERR_ARG, "x is NULL");
    if (B <= 0) return fail(VP3D_ERR_ASSERT, "batch must be positive");
    return calibrate_impl(h, x, B, T, stats_out, stream, nullptr);
}

int vp3d_x3_calibrate_windows(vp3d_handle* h, const float* kps, int32_t f2, const float* cams, const int64_t* seq_off,
                              const int32_t* seq_len, const int32_t* pairs, int B, int window, int lead,
                              vp3d_act_stats* stats_out, void* stream) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    if (!kps || !seq_off || !seq_len || !pairs) return fail(VP3D_ERR_ARG, "a device pointer is NULL");
    if (B <= 0) return fail(VP3D_ERR_ASSERT, "batch must be positive");
    const int cin = h->cfg.num_joints_in * h->cfg.in_features;
    if (f2 + (cams ? 12 : 0) != cin)
        return fail(VP3D_ERR_ASSERT, "frame features (" + std::to_string(f2) + (cams ? " + 12" : "") +
                                         ") != num_joints_in * in_features (" + std::to_string(cin) + ")");
    GatherSrc g;
    g.kps = kps;
    g.f2 = f2;
    g.cams = cams;
    g.seq_off = seq_off;
    g.seq_len = seq_len;
    g.pairs = pairs;
    g.lead = lead;
    return calibrate_impl(h, nullptr, B, window, stats_out, stream, &g);
}

int vp3d_profile_enable(vp3d_handle* h, int enable) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    h->profiling = enable != 0;
    return VP3D_OK;
}

int vp3d_profile_layers(vp3d_handle* h, uint64_t mask) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    h->prof_mask = mask;
    return VP3D_OK;
}

int vp3d_profile_reset(vp3d_handle* h) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    for (auto& e : h->pending) {
        hipEventSynchronize(e.b);
        h->free_events.push_back(e.a);
        h->free_events.push_back(e.b);
    }
    h->pending.clear();
    std::fill(h->prof_ms.begin(), h->prof_ms.end(), 0.0);
    std::fill(h->prof_n.begin(), h->prof_n.end(), 0);
    return VP3D_OK;
}

int vp3d_profile_read(vp3d_handle* h, double* ms_total, int64_t* launches, double* flop_last) {
    if (!h) return fail(VP3D_ERR_ARG, "handle is NULL");
    for (auto& e : h->pending) {
        HIP_TRY(hipEventSynchronize(e.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e.a, e.b));
        h->prof_ms[e.layer] += ms;
        h->prof_n[e.layer] += 1;
        h->prof_flop[e.layer] = e.flop;
        h->free_events.push_back(e.a);
        h->free_events.push_back(e.b);
    }
    h->pending.clear();
    for (size_t i = 0; i < h->layers.size(); ++i) {
        if (ms_total) ms_total[i] = h->prof_ms[i];
        if (launches) launches[i] = h->prof_n[i];
        if (flop_last) flop_last[i] = h->prof_flop[i];
    }
    return VP3D_OK;
}

// ---- causal streaming ----

}  // extern "C"

struct vp3d_stream {
    vp3d_handle* h = nullptr;
    int dtype = VP3D_DTYPE_F16;
    int* frames_seen = nullptr;        // device stream position + arrival counter
    float* in_frame = nullptr;         // device frame queue, kQueue x J_in*F
    float* out_pose = nullptr;         // device pose ring, kQueue x J_out*3
    int64_t host_t = 0;                // host mirror of the stream position
    int graph_steps = 0;
    float* rings = nullptr;            // all ring buffers
    float* scratch = nullptr;          // k-conv output, last block output
    std::vector<StreamLayerParams> steps;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    // persistent form (stream_persist.hip)
    bool persist = false;
    StreamPersistParams pp{};
    void* hand = nullptr;              // granules, zeroed before each launch
    size_t hand_bytes = 0;
    float* pstate = nullptr;           // per-workgroup partial rings + frame history
    // layer-pipelined form (stream_pipe.hip): preferred over `persist` when it fits
    bool pipe = false;
    StreamPipeParams pipe_p{};
    int pipe_lds = 0;
    unsigned long long* pipe_gran = nullptr;  // [queue][2nb+1][C] granules, cleared at reset
    size_t pipe_gran_bytes = 0;
    // serving with the shrink folded into the last block's 1x1 (StreamPipeParams::fold): the
    // host ring holds that role's partial sums, the host adds them with the shrink's scale / bias
    bool fold = false;
    int n_parts = 0;
    std::vector<float> shrink_scale, shrink_shift;
    unsigned long long* pipe_trace = nullptr;  // VP3D_STREAM_TRACE diagnostics
    float* pipe_state = nullptr;
    // persistent forms: host-mapped mirror of the sticky timeout word (frames_seen[3]), read
    // by step / graph_launch without a synchronisation
    unsigned* err_host = nullptr;
    unsigned* err_host_dev = nullptr;
    unsigned long long spin_ticks = kStreamSpinTicks;
    // serve form (pipe only): pinned host rings + control words, and the device end word
    bool serving = false;
    void* serve_host = nullptr;        // [ctrl: -, stop, ended][frame granules Q x cin][pose granules Q x nout]
    void* serve_dev = nullptr;         // device view of serve_host
    unsigned* end_frame = nullptr;     // device word
    int64_t posted = 0;                // host: frames posted so far (absolute)
    int64_t done_seen = 0;             // host: frames whose pose granules were all seen
    hipStream_t serve_stream = nullptr;
    // one event per HIP stream this vp3d_stream launched on, recorded after each launch:
    // vp3d_stream_reset waits for exactly these (not for the whole device)
    std::vector<std::pair<hipStream_t, hipEvent_t>> launch_events;
};

namespace {

constexpr int kQueue = 64;
constexpr const char* kStreamFaultMsg =
    "persistent stream step timed out waiting for another CU; the stream stays failed until vp3d_stream_reset";

int pow2_at_least(int v) {
    int r = 1;
    while (r < v) r <<= 1;
    return r;
}

// record "this vp3d_stream's launches on s are done" (not during a graph capture)
hipError_t mark_launched(vp3d_stream* st, hipStream_t s) {
    for (auto& se : st->launch_events)
        if (se.first == s) return hipEventRecord(se.second, s);
    hipEvent_t e = nullptr;
    hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r != hipSuccess) return r;
    st->launch_events.emplace_back(s, e);
    return hipEventRecord(e, s);
}

// `steps` consecutive steps: one persistent launch (after zeroing its hand-off words), or
// one GEMV launch per layer per step
int stream_launch(vp3d_stream* st, hipStream_t s, int steps = 1) {
    const Act wt = st->dtype == VP3D_DTYPE_F32 ? Act::F32 : (st->dtype == VP3D_DTYPE_BF16 ? Act::BF16 : Act::F16);
    if (st->pipe) {
        StreamPipeParams p = st->pipe_p;
        p.steps = steps;
        HIP_TRY(launch_stream_pipe(p, wt, st->pipe_lds, s));
        return VP3D_OK;
    }
    if (st->persist) {
        HIP_TRY(hipMemsetAsync(st->hand, 0, st->hand_bytes, s));
        StreamPersistParams p = st->pp;
        p.steps = steps;
        HIP_TRY(launch_stream_persist(p, wt, s));
        return VP3D_OK;
    }
    for (int i = 0; i < steps; ++i)
        for (const StreamLayerParams& q : st->steps) HIP_TRY(launch_stream_gemv(q, wt, s));
    return VP3D_OK;
}

// The persistent form's geometry: one workgroup per CU, CPW channels each, every LDS
// region 16-byte aligned.  False (the per-layer launches are used) when the model does
// not fit: fp32 weights, an expand width other than 3, more than kStreamMaxTaps taps,
// more than 4 channels per workgroup, or LDS over the kernel's budget.
bool stream_persist_setup(vp3d_stream* st, int dtype) {
    const vp3d_handle* h = st->h;
    if (dtype == VP3D_DTYPE_F32) return false;
    const char* mode = getenv("VP3D_STREAM_MODE");
    if (mode && !strcmp(mode, "launches")) return false;
    const int nl = (int)h->layers.size(), nb = h->cfg.n_widths - 1, C = h->cfg.channels;
    if (nl > kStreamMaxLayers || nb < 1 || nb > kStreamMaxBlocks) return false;
    if (h->layers[0].taps != 3 || h->layers[0].dil != 1) return false;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus < 1)
        return false;
    int CPW = (C + cus - 1) / cus;
    if (CPW > 4 || C % CPW) return false;
    StreamPersistParams& p = st->pp;
    p = StreamPersistParams{};
    p.nl = nl;
    p.nb = nb;
    p.C = C;
    p.CPW = CPW;
    p.G = C / CPW;
    p.cin0 = h->layers[0].cin;
    const int nout = h->layers[nl - 1].cout;
    if ((nout + CPW - 1) / CPW > p.G) return false;
    auto a16 = [](int v) { return (v + 15) / 16 * 16; };
    int off = 0;
    for (int l = 0; l < nl; ++l) {
        const Layer& L = h->layers[l];
        if (L.Kp % 8) return false;
        p.W[l] = dtype == VP3D_DTYPE_BF16 ? (const void*)L.wbf : (const void*)L.wh;
        p.scale[l] = L.scale;
        p.shift[l] = L.shift;
        p.Kp[l] = L.Kp;
        p.N[l] = L.cout;
        p.w_off[l] = off;
        off += a16(CPW * L.Kp * 2);
    }
    int part = 0;
    for (int b = 1; b <= nb; ++b) {
        const Layer& kc = h->layers[2 * b - 1];
        if (kc.taps > kStreamMaxTaps || kc.Ktap != C || kc.K != kc.taps * C) return false;
        p.taps[b] = kc.taps;
        p.dil[b] = kc.dil;
        p.ring[b] = pow2_at_least((kc.taps - 1) * kc.dil + 1);
        part += p.ring[b] * CPW;
    }
    p.x_off = off;
    off += a16(C * 4);
    p.xin_off = off;
    off += a16(h->layers[0].Kp * 4);
    p.hist_off = off;
    off += a16(2 * p.cin0 * 4);
    p.part_off = off;
    off += a16(part * 4);
    p.ss_off = off;
    off += a16(nl * 2 * CPW * 4);
    if (off > stream_persist_lds_bytes()) return false;
    p.part_floats = part;
    p.state_floats = part + 2 * p.cin0;
    p.frames = st->in_frame;
    p.queue = kQueue;
    p.poses = st->out_pose;
    p.frames_seen = st->frames_seen;
    st->hand_bytes = (size_t)(2 * nb + 1) * 2 * C * 8;
    if (hipMalloc(&st->hand, st->hand_bytes) != hipSuccess) return false;
    if (hipMalloc(&st->pstate, (size_t)p.G * p.state_floats * 4) != hipSuccess) {
        hipFree(st->hand);
        st->hand = nullptr;
        return false;
    }
    hipMemset(st->pstate, 0, (size_t)p.G * p.state_floats * 4);
    p.fault = StreamFault{(unsigned*)(st->frames_seen + 3), st->err_host_dev, st->spin_ticks};
    p.gran = (unsigned long long*)st->hand;
    p.state = st->pstate;
    return true;
}

// The layer-pipelined form's geometry (stream_pipe.hip): roles in layer order, each a
// contiguous range of workgroups (one per CU).  Expand: ceil(C / 256) workgroups (one
// channel per lane); shrink: ceil(N_out / 16); the rest split evenly over the blocks and,
// inside a block, about 3 : 1 between the k-conv (3 taps) and the 1x1 conv -- the ratio
// of their weights, so the per-frame work of the two groups is about equal.  False (the
// LDS-resident persistent form is tried next) for shapes the kernel does not cover:
// C other than 1024 / 256, k-convs other than 3 taps, an expand wider than 128 inputs.
bool stream_pipe_setup(vp3d_stream* st, int dtype) {
    const vp3d_handle* h = st->h;
    const char* mode = getenv("VP3D_STREAM_MODE");
    if (mode && strcmp(mode, "pipe")) return false;
    const int nl = (int)h->layers.size(), nb = h->cfg.n_widths - 1, C = h->cfg.channels;
    if (nl > kStreamMaxLayers || nb < 1 || nb > kStreamMaxBlocks || !stream_pipe_channels_ok(C)) return false;
    const Layer& e = h->layers[0];
    if (e.taps != 3 || e.dil != 1 || e.Kp > kPipeExpandK || e.cout != C) return false;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) return false;
    const int nout = h->layers[nl - 1].cout;
    const int n_e = (C + 255) / 256, n_s = (nout + 15) / 16;
    const int per_block = (cus - n_e - n_s) / nb;
    // channels are split over a role's workgroups in units of 8 (stream_pipe.hip); a workgroup
    // holds at most 8 waves x CW rows = CW units
    const int units = (C + 7) / 8;
    const int min_k = (units + kPipeCwK - 1) / kPipeCwK, min_p = (units + kPipeCwP - 1) / kPipeCwP;
    int n_p = std::max(min_p, per_block / 4);
    int n_k = per_block - n_p;
    n_k = std::min(n_k, std::max(min_k, C / 8));   // small models: fewer, fuller workgroups
    n_p = std::min(n_p, std::max(min_p, C / 16));
    if (n_k < min_k || ((nout + 7) / 8 + n_s - 1) / n_s > kPipeCwP) return false;
    StreamPipeParams& p = st->pipe_p;
    p = StreamPipeParams{};
    p.nl = nl;
    p.nb = nb;
    p.C = C;
    p.cin0 = e.cin;
    int max_ring = 1;
    for (int b = 1; b <= nb; ++b) {
        const Layer& kc = h->layers[2 * b - 1];
        const Layer& pc = h->layers[2 * b];
        if (kc.taps != 3 || kc.Ktap != C || kc.K != 3 * C || kc.cout != C || pc.K != C || pc.cout != C) return false;
        p.dil[b] = kc.dil;
        p.ring[b] = pow2_at_least(2 * kc.dil + 1);
        max_ring = std::max(max_ring, p.ring[b]);
    }
    if (h->layers[nl - 1].K != C) return false;
    int g = 0;
    for (int l = 0; l < nl; ++l) {
        const Layer& L = h->layers[l];
        p.W[l] = dtype == VP3D_DTYPE_F32 ? (const void*)L.w32
                 : dtype == VP3D_DTYPE_BF16 ? (const void*)L.wbf : (const void*)L.wh;
        p.scale[l] = L.scale;
        p.shift[l] = L.shift;
        p.Kp[l] = L.Kp;
        p.N[l] = L.cout;
        p.cu0[l] = g;
        g += l == 0 ? n_e : (l == nl - 1 ? n_s : (l & 1 ? n_k : n_p));
    }
    p.cu0[nl] = g;
    if (g > cus) return false;
    const int lds = stream_pipe_lds_bytes(C, p.cin0, max_ring);
    const Act wt = dtype == VP3D_DTYPE_F32 ? Act::F32 : (dtype == VP3D_DTYPE_BF16 ? Act::BF16 : Act::F16);
    if (lds > 160 * 1024 || stream_pipe_prepare(wt, C, lds) != hipSuccess) return false;
    st->pipe_lds = lds;
    p.state_stride = std::max(8 * max_ring * kPipeCwK, 2 * p.cin0);
    // hand-off layout and polling (defaults measured in round 3, tools/stream_latency.py)
    p.chunk_stride = 64;
    p.poll_pause = 1;
    // contiguous rows: a wave's outputs are neighbouring granules stored by one instruction
    // (strided rows put 8 waves' stores into every 64-byte line: hand-offs 0.4-1.0 us slower)
    p.row_contig = 1;
    if (const char* e = getenv("VP3D_STREAM_ROWS")) p.row_contig = strcmp(e, "strided") != 0;
    if (const char* e = getenv("VP3D_STREAM_CHUNK_STRIDE")) p.chunk_stride = std::max(64, atoi(e));
    if (const char* e = getenv("VP3D_STREAM_POLL_PAUSE")) p.poll_pause = std::min(64, std::max(0, atoi(e)));
    st->pipe_gran_bytes = (size_t)kQueue * (2 * nb + 1) * (C / 64) * p.chunk_stride * 8;
    if (hipMalloc(&st->pipe_gran, st->pipe_gran_bytes) != hipSuccess) return false;
    if (hipMalloc(&st->pipe_state, (size_t)g * p.state_stride * 4) != hipSuccess) {
        hipFree(st->pipe_gran);
        st->pipe_gran = nullptr;
        return false;
    }
    hipMemset(st->pipe_gran, 0, st->pipe_gran_bytes);
    hipMemset(st->pipe_state, 0, (size_t)g * p.state_stride * 4);
    // serving: the shrink folded into the last block's 1x1 (VP3D_STREAM_FOLD=0 keeps the shrink
    // role's all-gather): that role's workgroups cover <= 64 channels each (8 waves x 8 rows)
    // and the outputs fit one 64-granule slot per workgroup
    {
        const int np = p.cu0[nl - 1] - p.cu0[nl - 2];
        const char* fe = getenv("VP3D_STREAM_FOLD");
        const bool want = !(fe && fe[0] == '0');
        if (want && nout <= 64 && np >= 1 && np <= 64) {
            const Layer& sl = h->layers[nl - 1];
            st->shrink_scale.assign(nout, 0.f);
            st->shrink_shift.assign(nout, 0.f);
            if (hipMemcpy(st->shrink_scale.data(), sl.scale, 4 * nout, hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(st->shrink_shift.data(), sl.shift, 4 * nout, hipMemcpyDeviceToHost) == hipSuccess) {
                st->fold = true;
                st->n_parts = np;
                p.fold = 1;
            }
        }
    }
    p.frames = st->in_frame;
    p.queue = kQueue;
    p.poses = st->out_pose;
    p.frames_seen = st->frames_seen;
    p.arrivals = (unsigned*)(st->frames_seen + 2);
    p.fault = StreamFault{(unsigned*)(st->frames_seen + 3), st->err_host_dev, st->spin_ticks};
    p.gran = st->pipe_gran;
    p.state = st->pipe_state;
    if (const char* e = getenv("VP3D_STREAM_TRACE")) {
        const int n = atoi(e);
        const size_t tb = (size_t)g * n * kStreamTraceSlots * 8;
        if (n > 0 && hipMalloc(&st->pipe_trace, tb) == hipSuccess) {
            hipMemset(st->pipe_trace, 0, tb);
            p.trace = st->pipe_trace;
            p.trace_frames = n;
        }
    }
    return true;
}

}  // namespace

extern "C" {

int vp3d_stream_create(vp3d_handle* h, int dtype, vp3d_stream** out) {
    if (!h || !out) return fail(VP3D_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (dtype < 0 || dtype > 2) return fail(VP3D_ERR_ARG, "unknown dtype");
    if (h->cfg.variant != VP3D_VARIANT_DILATED || !h->cfg.causal)
        return fail(VP3D_ERR_ARG, "streaming needs a causal dilated TemporalModel");
    for (const Layer& L : h->layers)
        if (L.Kp > 4096) return fail(VP3D_ERR_ARG, "streaming supports K <= 4096 per layer");
    int dev = 0;
    hipGetDevice(&dev);
    if (dev != h->device) return fail(VP3D_ERR_STATE, "handle belongs to another device");

    vp3d_stream* st = new vp3d_stream();
    st->h = h;
    st->dtype = dtype;
    const int C = h->cfg.channels;
    const int nl = (int)h->layers.size();
    const int nb = h->cfg.n_widths - 1;
    // ring i holds the input of layer (expand: raw frames) / block i
    std::vector<int> ring_len, ring_width;
    ring_len.push_back(pow2_at_least((h->layers[0].taps - 1) * h->layers[0].dil + 1));
    ring_width.push_back(h->layers[0].cin);
    for (int b = 1; b <= nb; ++b) {
        const Layer& kc = h->layers[2 * b - 1];
        ring_len.push_back(pow2_at_least((kc.taps - 1) * kc.dil + 1));
        ring_width.push_back(C);
    }
    size_t ring_floats = 0;
    std::vector<size_t> ring_off;
    for (size_t i = 0; i < ring_len.size(); ++i) {
        ring_off.push_back(ring_floats);
        ring_floats += (size_t)ring_len[i] * ring_width[i];
    }
    auto cleanup = [&](int rc) {
        hipFree(st->frames_seen);
        hipFree(st->in_frame);
        hipFree(st->out_pose);
        hipFree(st->rings);
        hipFree(st->scratch);
        delete st;
        return rc;
    };
    if (hipMalloc(&st->frames_seen, 16) != hipSuccess ||
        hipMalloc(&st->in_frame, 4 * (size_t)kQueue * h->layers[0].cin) != hipSuccess ||
        hipMalloc(&st->out_pose, 4 * (size_t)kQueue * h->layers.back().cout) != hipSuccess ||
        hipMalloc(&st->rings, 4 * ring_floats) != hipSuccess || hipMalloc(&st->scratch, 8 * (size_t)C) != hipSuccess)
        return cleanup(fail(VP3D_ERR_OOM, "stream buffers"));
    hipMemset(st->frames_seen, 0, 16);
    hipMemset(st->rings, 0, 4 * ring_floats);
    float* hbuf = st->scratch;           // k-conv output of the current block
    float* xlast = st->scratch + C;      // output of the last block (or of expand if nb == 0)

    auto W = [&](const Layer& L) -> const void* {
        return dtype == VP3D_DTYPE_F32 ? (const void*)L.w32 : (dtype == VP3D_DTYPE_BF16 ? (const void*)L.wbf : (const void*)L.wh);
    };
    auto base = [&](const Layer& L) {
        StreamLayerParams q{};
        q.W = W(L);
        q.scale = L.scale;
        q.shift = L.shift;
        q.N = L.cout;
        q.K = L.K;
        q.Kp = L.Kp;
        q.cin = L.cin;
        q.taps = L.taps;
        q.dil = L.dil;
        q.relu = L.relu ? 1 : 0;
        q.frames_seen = st->frames_seen;
        return q;
    };
    // expand: raw-frame ring 0 (+ the new frame) -> ring 1 (block 1 input)
    {
        StreamLayerParams q = base(h->layers[0]);
        q.in = st->rings + ring_off[0];
        q.in_R = ring_len[0];
        q.in_frame = st->in_frame;
        q.in_frame_R = kQueue;
        q.in_ring_w = st->rings + ring_off[0];
        if (nb > 0) {
            q.out = st->rings + ring_off[1];
            q.out_R = ring_len[1];
        } else {
            q.out = xlast;
        }
        st->steps.push_back(q);
    }
    for (int b = 1; b <= nb; ++b) {
        StreamLayerParams k = base(h->layers[2 * b - 1]);
        k.in = st->rings + ring_off[b];
        k.in_R = ring_len[b];
        k.out = hbuf;
        st->steps.push_back(k);
        StreamLayerParams pw = base(h->layers[2 * b]);
        pw.in = hbuf;
        pw.res = st->rings + ring_off[b];
        pw.res_R = ring_len[b];
        if (b < nb) {
            pw.out = st->rings + ring_off[b + 1];
            pw.out_R = ring_len[b + 1];
        } else {
            pw.out = xlast;
        }
        st->steps.push_back(pw);
    }
    {
        StreamLayerParams q = base(h->layers[nl - 1]);
        q.in = xlast;
        q.out = st->out_pose;
        q.out_R = kQueue;
        q.advance = 1;
        q.done_counter = (unsigned*)(st->frames_seen + 1);
        st->steps.push_back(q);
    }
    if (const char* e = getenv("VP3D_STREAM_SPIN_TICKS")) st->spin_ticks = strtoull(e, nullptr, 10);
    if (hipHostMalloc(&st->err_host, 4, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&st->err_host_dev, st->err_host, 0) != hipSuccess) {
        hipHostFree(st->err_host);
        return cleanup(fail(VP3D_ERR_OOM, "stream fault word"));
    }
    *(volatile unsigned*)st->err_host = 0u;
    st->pipe = stream_pipe_setup(st, dtype);
    if (!st->pipe) st->persist = stream_persist_setup(st, dtype);
    hipDeviceSynchronize();  // setup memsets (legacy stream) before any launch on another stream
    *out = st;
    return VP3D_OK;
}

int vp3d_stream_persistent(const vp3d_stream* st) { return st && (st->persist || st->pipe) ? 1 : 0; }

int vp3d_stream_mode(const vp3d_stream* st) { return !st ? -1 : st->pipe ? 2 : st->persist ? 1 : 0; }

int vp3d_stream_status(vp3d_stream* st) {
    if (!st) return fail(VP3D_ERR_ARG, "stream is NULL");
    if (!st->persist && !st->pipe) return VP3D_OK;
    unsigned err = 0;
    HIP_TRY(hipMemcpy(&err, (void*)(st->frames_seen + 3), 4, hipMemcpyDeviceToHost));
    if (err) return fail(VP3D_ERR_STATE, kStreamFaultMsg);
    return VP3D_OK;
}

int vp3d_stream_reset(vp3d_stream* st, void* stream) {
    if (!st) return fail(VP3D_ERR_ARG, "stream is NULL");
    if (st->serving) return fail(VP3D_ERR_STATE, "serving: vp3d_stream_serve_end first");
    // position, arrival counter and the sticky timeout word; the host mirror is cleared
    // once no launch of this stream can still set it (launches may have gone to any stream:
    // wait for each one's last launch, not for the whole device)
    for (auto& se : st->launch_events) HIP_TRY(hipEventSynchronize(se.second));
    HIP_TRY(hipMemsetAsync(st->frames_seen, 0, 16, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    *(volatile unsigned*)st->err_host = 0u;
    // pipelined form: granule tags restart at frame 1
    if (st->pipe) HIP_TRY(hipMemsetAsync(st->pipe_gran, 0, st->pipe_gran_bytes, (hipStream_t)stream));
    st->host_t = 0;
    return VP3D_OK;
}

int vp3d_stream_io(vp3d_stream* st, float** in_frames, float** out_poses, int* queue_len) {
    if (!st) return fail(VP3D_ERR_ARG, "stream is NULL");
    if (in_frames) *in_frames = st->in_frame;
    if (out_poses) *out_poses = st->out_pose;
    if (queue_len) *queue_len = kQueue;
    return VP3D_OK;
}

int vp3d_stream_step(vp3d_stream* st, const float* frame, float* pose, void* stream) {
    if (!st) return fail(VP3D_ERR_ARG, "stream is NULL");
    if (st->serving) return fail(VP3D_ERR_STATE, "serving: post frames with vp3d_stream_serve_post");
    if (*(volatile unsigned*)st->err_host) return fail(VP3D_ERR_STATE, kStreamFaultMsg);
    hipStream_t s = (hipStream_t)stream;
    const int slot = (int)(st->host_t % kQueue);
    const int cin = st->h->layers[0].cin, cout = st->h->layers.back().cout;
    if (frame)
        HIP_TRY(hipMemcpyAsync(st->in_frame + (size_t)slot * cin, frame, 4 * cin,
                               hipMemcpyDeviceToDevice, s));
    int rc = stream_launch(st, s);
    if (rc) return rc;
    HIP_TRY(mark_launched(st, s));
    if (pose)
        HIP_TRY(hipMemcpyAsync(pose, st->out_pose + (size_t)slot * cout, 4 * cout,
                               hipMemcpyDeviceToDevice, s));
    st->host_t += 1;
    return VP3D_OK;
}

int64_t vp3d_stream_frames_seen(vp3d_stream* st) {
    if (!st) return -1;
    int v = -1;
    if (hipMemcpy(&v, st->frames_seen, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v;
}

int vp3d_stream_graph_capture(vp3d_stream* st, void* stream, int steps) {
    if (!st) return fail(VP3D_ERR_ARG, "stream is NULL");
    if (!stream) return fail(VP3D_ERR_ARG, "graph capture needs a non-default stream");
    if (steps < 1) return fail(VP3D_ERR_ARG, "steps must be >= 1");
    hipStream_t s = (hipStream_t)stream;
    if (st->exec) {
        hipGraphExecDestroy(st->exec);
        st->exec = nullptr;
    }
    if (st->graph) {
        hipGraphDestroy(st->graph);
        st->graph = nullptr;
    }
    if ((st->persist || st->pipe) && steps > kQueue) return fail(VP3D_ERR_ARG, "a persistent graph runs at most queue_len steps");
    HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = stream_launch(st, s, steps);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(s, &g);
    if (rc) return rc;
    if (e != hipSuccess) return fail(VP3D_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    st->graph = g;
    st->graph_steps = steps;
    HIP_TRY(hipGraphInstantiate(&st->exec, g, nullptr, nullptr, 0));
    return VP3D_OK;
}

int vp3d_stream_graph_launch(vp3d_stream* st, void* stream) {
    if (!st || !st->exec) return fail(VP3D_ERR_STATE, "no captured graph");
    if (st->serving) return fail(VP3D_ERR_STATE, "serving: post frames with vp3d_stream_serve_post");
    if (*(volatile unsigned*)st->err_host) return fail(VP3D_ERR_STATE, kStreamFaultMsg);
    HIP_TRY(hipGraphLaunch(st->exec, (hipStream_t)stream));
    HIP_TRY(mark_launched(st, (hipStream_t)stream));
    st->host_t += st->graph_steps;
    return VP3D_OK;
}

}  // extern "C"

namespace {
constexpr int kServeCtrlWords = 32;  // [1] stop, [2] ended (+1); 128 bytes, so the rings stay 8-byte aligned
unsigned* serve_ctrl(vp3d_stream* st) { return (unsigned*)st->serve_host; }
// {tag = frame + 1, f32 bits} granules: frame t in slot t % Q of each ring
uint64_t* serve_frames(vp3d_stream* st) { return (uint64_t*)((char*)st->serve_host + kServeCtrlWords * 4); }
uint64_t* serve_poses(vp3d_stream* st) { return serve_frames(st) + (size_t)kQueue * st->h->layers[0].cin; }
// granules per frame slot of the host pose ring: the poses, or with the shrink folded the last
// block's partial sums (n_parts x 64)
size_t serve_pose_slot(const vp3d_stream* st) {
    return st->fold ? (size_t)st->n_parts * 64 : (size_t)st->h->layers.back().cout;
}
template <typename T>
T* dev_view(vp3d_stream* st, T* host_ptr) {
    return (T*)((char*)st->serve_dev + ((char*)host_ptr - (char*)st->serve_host));
}
// every pose granule of frame f carries its tag (the shrink workgroups store them last)
bool serve_pose_ready(vp3d_stream* st, int64_t f) {
    const int nout = st->h->layers.back().cout;
    const uint64_t* g = serve_poses(st) + (size_t)(f % kQueue) * serve_pose_slot(st);
    const int parts = st->fold ? st->n_parts : 1;
    for (int w = 0; w < parts; ++w)
        for (int i = 0; i < nout; ++i)
            if ((uint32_t)(__atomic_load_n(g + (size_t)w * 64 + i, __ATOMIC_RELAXED) >> 32) != (uint32_t)(f + 1))
                return false;
    return true;
}
// frames complete in order: advance the host's count of finished frames
int64_t serve_done(vp3d_stream* st) {
    while (st->done_seen < st->posted && serve_pose_ready(st, st->done_seen)) ++st->done_seen;
    return st->done_seen;
}
}  // namespace

extern "C" {

int vp3d_stream_serve_begin(vp3d_stream* st, void* stream, double idle_ms) {
    if (!st) return fail(VP3D_ERR_ARG, "stream is NULL");
    if (!st->pipe) return fail(VP3D_ERR_STATE, "serving needs the layer-pipelined form (vp3d_stream_mode 2)");
    if (st->serving) return fail(VP3D_ERR_STATE, "already serving");
    if (*(volatile unsigned*)st->err_host) return fail(VP3D_ERR_STATE, kStreamFaultMsg);
    if (!(idle_ms > 0.0) || idle_ms > 1000.0) return fail(VP3D_ERR_ARG, "idle_ms must be in (0, 1000]");
    hipStream_t s = (hipStream_t)stream;
    const vp3d_handle* h = st->h;
    const size_t bytes = kServeCtrlWords * 4 + (size_t)kQueue * (h->layers[0].cin + serve_pose_slot(st)) * 8;
    if (!st->serve_host) {
        HIP_TRY(hipHostMalloc(&st->serve_host, bytes, hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer(&st->serve_dev, st->serve_host, 0));
        HIP_TRY(hipMalloc(&st->end_frame, 8));  // [0] end frame, [1] the expand role's claim word
    }
    // the stream position of the device (any earlier launches on `stream` finished)
    HIP_TRY(hipStreamSynchronize(s));
    if (st->fold) {
        // the host-side shrink affine of the folded form, from the handle's CURRENT weights:
        // vp3d_load_weights rewrites them in place after the stream was created, and the
        // resident launch below loads the other layers' weights now too
        const Layer& sl = h->layers.back();
        const int nout = sl.cout;
        HIP_TRY(hipMemcpy(st->shrink_scale.data(), sl.scale, 4 * nout, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(st->shrink_shift.data(), sl.shift, 4 * nout, hipMemcpyDeviceToHost));
    }
    int pos = 0;
    HIP_TRY(hipMemcpy(&pos, st->frames_seen, 4, hipMemcpyDeviceToHost));
    st->host_t = pos;
    st->posted = pos;
    st->done_seen = pos;
    // no granule of an earlier session (or of frames before a reset) may carry a tag of this one
    std::memset(st->serve_host, 0, bytes);
    const unsigned ctl[2] = {0xFFFFFFFFu, (unsigned)pos};  // not ended; frames before pos committed
    HIP_TRY(hipMemcpy(st->end_frame, ctl, 8, hipMemcpyHostToDevice));
    StreamPipeParams p = st->pipe_p;
    p.serve = 1;
    p.frame_gran = (const unsigned long long*)dev_view(st, serve_frames(st));
    p.pose_gran = (unsigned long long*)dev_view(st, serve_poses(st));
    p.stop = dev_view(st, serve_ctrl(st) + 1);
    p.ended_host = dev_view(st, serve_ctrl(st) + 2);
    p.end_frame = st->end_frame;
    p.end_claim = st->end_frame + 1;
    p.idle_ticks = (unsigned long long)(idle_ms * 1e5);  // 100 MHz clock
    p.steps = 0;
    const Act wt = st->dtype == VP3D_DTYPE_F32 ? Act::F32 : (st->dtype == VP3D_DTYPE_BF16 ? Act::BF16 : Act::F16);
    HIP_TRY(launch_stream_pipe(p, wt, st->pipe_lds, s));
    HIP_TRY(mark_launched(st, s));
    st->serving = true;
    st->serve_stream = s;
    return VP3D_OK;
}

int vp3d_stream_serve_post(vp3d_stream* st, const float* frame, int64_t* frame_index) {
    if (!st || !frame) return fail(VP3D_ERR_ARG, "NULL argument");
    if (!st->serving) return fail(VP3D_ERR_STATE, "not serving (vp3d_stream_serve_begin)");
    if (*(volatile unsigned*)st->err_host) return fail(VP3D_ERR_STATE, kStreamFaultMsg);
    if (((volatile unsigned*)serve_ctrl(st))[2]) return fail(VP3D_ERR_STATE, "the serve launch ended (idle); vp3d_stream_serve_end, then begin");
    if (st->posted - serve_done(st) >= kQueue - 1)
        return fail(VP3D_ERR_STATE, "serve ring full: wait for earlier frames first");
    const int cin = st->h->layers[0].cin;
    const int64_t t = st->posted;
    // one 8-byte store per value: the expand workgroups poll these granules themselves
    uint64_t* g = serve_frames(st) + (size_t)(t % kQueue) * cin;
    const uint64_t tag = (uint64_t)(uint32_t)(t + 1) << 32;
    for (int i = 0; i < cin; ++i) {
        uint32_t bits;
        std::memcpy(&bits, frame + i, 4);
        __atomic_store_n(g + i, tag | bits, __ATOMIC_RELAXED);
    }
    st->posted = t + 1;
    if (frame_index) *frame_index = t;
    return VP3D_OK;
}

int vp3d_stream_serve_wait(vp3d_stream* st, int64_t frame_index, float* pose, double timeout_ms) {
    if (!st) return fail(VP3D_ERR_ARG, "stream is NULL");
    if (!st->serving) return fail(VP3D_ERR_STATE, "not serving (vp3d_stream_serve_begin)");
    if (frame_index < 0 || frame_index >= st->posted) return fail(VP3D_ERR_ARG, "frame was not posted");
    if (st->posted - frame_index >= kQueue) return fail(VP3D_ERR_ARG, "frame's pose slot was reused");
    const auto t0 = std::chrono::steady_clock::now();
    // a cursor over the frame's granules: each poll resumes at the first one not yet seen
    // (with the shrink folded, 16 x 51 partials: re-reading those already seen every poll
    // was host time on the frame's path)
    const int nout_w = st->h->layers.back().cout;
    const int parts_w = st->fold ? st->n_parts : 1;
    const uint64_t* gw = serve_poses(st) + (size_t)(frame_index % kQueue) * serve_pose_slot(st);
    int cw = 0, ci = 0;
    for (;;) {
        while (cw < parts_w &&
               (uint32_t)(__atomic_load_n(gw + (size_t)cw * 64 + ci, __ATOMIC_RELAXED) >> 32) == (uint32_t)(frame_index + 1)) {
            if (++ci == nout_w) {
                ci = 0;
                ++cw;
            }
        }
        if (cw == parts_w) break;
        if (*(volatile unsigned*)st->err_host) return fail(VP3D_ERR_STATE, kStreamFaultMsg);
        const unsigned ended = ((volatile unsigned*)serve_ctrl(st))[2];
        if (ended && (int64_t)ended - 1 <= frame_index) return fail(VP3D_ERR_STATE, "the serve launch ended before this frame");
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms > timeout_ms) return fail(VP3D_ERR_STATE, "serve wait timed out (the launch ended or is stalled)");
    }
    const int nout = st->h->layers.back().cout;
    const uint64_t* g = serve_poses(st) + (size_t)(frame_index % kQueue) * serve_pose_slot(st);
    auto val = [&](size_t i) {
        const uint32_t bits = (uint32_t)__atomic_load_n(g + i, __ATOMIC_RELAXED);
        float v;
        std::memcpy(&v, &bits, 4);
        return v;
    };
    if (pose) {
        if (st->fold) {
            // the shrink folded into the last 1x1 group: its per-workgroup partial sums added
            // here in workgroup order, then the affine.  The graph form's shrink sums the same
            // products in another order, so served poses match it within 1e-6 m, not bit for
            // bit (deterministic from run to run)
            for (int i = 0; i < nout; ++i) {
                float a = val(i);
                for (int w = 1; w < st->n_parts; ++w) a += val((size_t)w * 64 + i);
                const float sa = a * st->shrink_scale[i];
                pose[i] = sa + st->shrink_shift[i];
            }
        } else {
            for (int i = 0; i < nout; ++i) pose[i] = val(i);
        }
    }
    return VP3D_OK;
}

int vp3d_stream_serve_step(vp3d_stream* st, const float* frame, float* pose, double timeout_ms, double* latency_us) {
    const auto t0 = std::chrono::steady_clock::now();
    int64_t t = 0;
    int rc = vp3d_stream_serve_post(st, frame, &t);
    if (rc != VP3D_OK) return rc;
    rc = vp3d_stream_serve_wait(st, t, pose, timeout_ms);
    if (latency_us)
        *latency_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int vp3d_stream_serve_end(vp3d_stream* st, void* stream) {
    if (!st) return fail(VP3D_ERR_ARG, "stream is NULL");
    if (!st->serving) return VP3D_OK;
    __atomic_store_n(serve_ctrl(st) + 1, 1u, __ATOMIC_RELEASE);
    st->serving = false;
    // the resident launch runs on the stream serve_begin was given, whatever `stream` is
    (void)stream;
    HIP_TRY(hipStreamSynchronize(st->serve_stream));
    int pos = 0;
    HIP_TRY(hipMemcpy(&pos, st->frames_seen, 4, hipMemcpyDeviceToHost));
    st->host_t = pos;
    if (*(volatile unsigned*)st->err_host) return fail(VP3D_ERR_STATE, kStreamFaultMsg);
    return VP3D_OK;
}

int vp3d_stream_trace(vp3d_stream* st, uint64_t* out, int64_t capacity, int32_t* role_first_wg, int32_t* n_roles,
                      int32_t* frames) {
    if (!st || !n_roles || !frames) return fail(VP3D_ERR_ARG, "NULL argument");
    if (!st->pipe_trace) return fail(VP3D_ERR_STATE, "no trace: set VP3D_STREAM_TRACE=n before vp3d_stream_create");
    const StreamPipeParams& p = st->pipe_p;
    *n_roles = p.nl;
    *frames = p.trace_frames;
    if (role_first_wg)
        for (int l = 0; l <= p.nl; ++l) role_first_wg[l] = p.cu0[l];
    const int64_t need = (int64_t)p.cu0[p.nl] * p.trace_frames * kStreamTraceSlots;
    if (!out) return VP3D_OK;
    if (capacity < need) return fail(VP3D_ERR_ARG, "trace buffer too small");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, st->pipe_trace, (size_t)need * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(st->pipe_trace, 0, (size_t)need * 8));
    return VP3D_OK;
}

int vp3d_stream_destroy(vp3d_stream* st) {
    if (!st) return VP3D_OK;
    if (st->serving) vp3d_stream_serve_end(st, nullptr);
    hipHostFree(st->serve_host);
    hipFree(st->end_frame);
    if (st->exec) hipGraphExecDestroy(st->exec);
    if (st->graph) hipGraphDestroy(st->graph);
    hipFree(st->frames_seen);
    hipFree(st->in_frame);
    hipFree(st->out_pose);
    hipFree(st->rings);
    hipFree(st->scratch);
    hipFree(st->hand);
    hipFree(st->pstate);
    hipFree(st->pipe_gran);
    hipFree(st->pipe_state);
    hipFree(st->pipe_trace);
    hipHostFree(st->err_host);
    for (auto& se : st->launch_events) hipEventDestroy(se.second);
    delete st;
    return VP3D_OK;
}

// ---- batched causal streaming (stream_batch.hip) ----

}  // extern "C"

struct vp3d_mstream {
    vp3d_handle* h = nullptr;
    int dtype = VP3D_DTYPE_F16;
    int S = 0;
    int* pos = nullptr;        // device: [S] stream positions, then [S] the step's active words
    float* frames = nullptr;   // device io: (S, J_in*F)
    float* poses = nullptr;    // device io: (S, J_out*3)
    float* rings = nullptr;    // S x (every ring of one stream)
    float* scratch = nullptr;  // S x C k-conv outputs, then S x C last-block outputs
    std::vector<StreamBatchParams> steps;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    // look-ahead form (vp3d_lstream): pos then also holds [S] frames consumed and [S] pose_frame,
    // and the active words are step codes
    bool look = false;
    int lookahead = 0;
};

// a vp3d_mstream of the look-ahead form behind its own opaque type
struct vp3d_lstream {
    vp3d_mstream* m = nullptr;
};

namespace {

int32_t* mstream_active(vp3d_mstream* m) { return (int32_t*)(m->pos + m->S); }
int* mstream_consumed(vp3d_mstream* m) { return m->pos + 2 * m->S; }
int32_t* mstream_pose_frame(vp3d_mstream* m) { return (int32_t*)(m->pos + 3 * m->S); }

// one step on the io buffers: a launch per layer, then the positions
int mstream_launch(vp3d_mstream* m, hipStream_t s) {
    const Act wt = m->dtype == VP3D_DTYPE_F32 ? Act::F32 : (m->dtype == VP3D_DTYPE_BF16 ? Act::BF16 : Act::F16);
    for (const StreamBatchParams& q : m->steps) HIP_TRY(launch_stream_batch(q, wt, s));
    if (m->look)
        HIP_TRY(launch_stream_batch_advance_look(m->pos, mstream_consumed(m), mstream_active(m), mstream_pose_frame(m),
                                                 m->lookahead, m->S, s));
    else
        HIP_TRY(launch_stream_batch_advance(m->pos, mstream_active(m), m->S, s));
    return VP3D_OK;
}

void mstream_free(vp3d_mstream* m) {
    if (m->exec) hipGraphExecDestroy(m->exec);
    if (m->graph) hipGraphDestroy(m->graph);
    hipFree(m->pos);
    hipFree(m->frames);
    hipFree(m->poses);
    hipFree(m->rings);
    hipFree(m->scratch);
    delete m;
}

// the buffers and per-layer launch parameters of a batched stream; look: the look-ahead form of
// a non-causal model (vp3d_lstream), else the causal one (vp3d_mstream)
int mstream_build(vp3d_handle* h, int dtype, int n_streams, bool look, vp3d_mstream** out) {
    if (!h || !out) return fail(VP3D_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (dtype < 0 || dtype > 2) return fail(VP3D_ERR_ARG, "unknown dtype");
    if (n_streams < 1 || n_streams > VP3D_MSTREAM_MAX)
        return fail(VP3D_ERR_ARG, "n_streams must be 1.." + std::to_string(VP3D_MSTREAM_MAX));
    static_assert(VP3D_MSTREAM_MAX == kStreamBatchMax, "the kernel's slot limit is the ABI's");
    if (look) {
        if (h->cfg.variant != VP3D_VARIANT_DILATED)
            return fail(VP3D_ERR_ARG, "look-ahead streaming needs a dilated TemporalModel (not the strided variant)");
        if (h->cfg.causal) return fail(VP3D_ERR_ARG, "causal TemporalModel, look-ahead 0: use vp3d_mstream");
    } else if (h->cfg.variant != VP3D_VARIANT_DILATED || !h->cfg.causal) {
        return fail(VP3D_ERR_ARG, "streaming needs a causal dilated TemporalModel");
    }
    for (const Layer& L : h->layers)
        if (L.Kp > 4096) return fail(VP3D_ERR_ARG, "streaming supports K <= 4096 per layer");
    int dev = 0;
    hipGetDevice(&dev);
    if (dev != h->device) return fail(VP3D_ERR_STATE, "handle belongs to another device");

    vp3d_mstream* m = new vp3d_mstream();
    m->h = h;
    m->dtype = dtype;
    m->S = n_streams;
    m->look = look;
    for (int p : h->pad) m->lookahead += look ? p : 0;
    const size_t pos_bytes = (look ? 16 : 8) * (size_t)n_streams;
    const int S = n_streams;
    const int C = h->cfg.channels;
    const int nl = (int)h->layers.size();
    const int nb = h->cfg.n_widths - 1;
    const int cin0 = h->layers[0].cin, nout = h->layers.back().cout;
    // ring i of a slot holds the input of layer (expand: raw frames) / block i, the single
    // stream's sizes; offsets rounded to 16 bytes so that rows of 4 | cin floats stay aligned
    std::vector<int> ring_len;
    std::vector<size_t> ring_off;
    size_t ring_floats = 0;
    auto add_ring = [&](const Layer& L, int width) {
        ring_len.push_back(pow2_at_least((L.taps - 1) * L.dil + 1));
        ring_off.push_back(ring_floats);
        ring_floats += ((size_t)ring_len.back() * width + 3) / 4 * 4;
    };
    add_ring(h->layers[0], cin0);
    for (int b = 1; b <= nb; ++b) add_ring(h->layers[2 * b - 1], C);
    if (hipMalloc(&m->pos, pos_bytes) != hipSuccess || hipMalloc(&m->frames, 4 * (size_t)S * cin0) != hipSuccess ||
        hipMalloc(&m->poses, 4 * (size_t)S * nout) != hipSuccess ||
        hipMalloc(&m->rings, 4 * (size_t)S * ring_floats) != hipSuccess ||
        hipMalloc(&m->scratch, 8 * (size_t)S * C) != hipSuccess) {
        mstream_free(m);
        return fail(VP3D_ERR_OOM, "batched stream buffers");
    }
    hipMemset(m->pos, 0, pos_bytes);
    if (look) hipMemset(mstream_pose_frame(m), 0xff, 4 * (size_t)S);  // -1: no pose row written yet
    hipMemset(m->frames, 0, 4 * (size_t)S * cin0);
    hipMemset(m->poses, 0, 4 * (size_t)S * nout);
    hipMemset(m->rings, 0, 4 * (size_t)S * ring_floats);
    float* hbuf = m->scratch;                  // (S, C) k-conv output of the current block
    float* xlast = m->scratch + (size_t)S * C;  // (S, C) output of the last block (or of expand if nb == 0)

    auto base = [&](const Layer& L) {
        StreamBatchParams q{};
        q.W = dtype == VP3D_DTYPE_F32 ? (const void*)L.w32 : (dtype == VP3D_DTYPE_BF16 ? (const void*)L.wbf : (const void*)L.wh);
        q.scale = L.scale;
        q.shift = L.shift;
        q.N = L.cout;
        q.K = L.K;
        q.Kp = L.Kp;
        q.cin = L.cin;
        q.taps = L.taps;
        q.dil = L.dil;
        q.relu = L.relu ? 1 : 0;
        q.S = S;
        q.t = m->pos;
        q.active = mstream_active(m);
        if (look) {
            q.n = mstream_consumed(m);
            q.lookahead = m->lookahead;
        }
        return q;
    };
    auto ring_in = [&](StreamBatchParams& q, int i) {
        q.in = m->rings + ring_off[i];
        q.in_R = ring_len[i];
        q.in_stride = (int64_t)ring_floats;
    };
    auto plain_in = [&](StreamBatchParams& q, const float* v) {
        q.in = v;
        q.in_stride = C;
    };
    // the output of the layer that feeds block b (ring b), or the last block's plain rows
    auto out_to = [&](StreamBatchParams& q, int b) {
        if (b <= nb) {
            q.out = m->rings + ring_off[b];
            q.out_R = ring_len[b];
            q.out_stride = (int64_t)ring_floats;
        } else {
            q.out = xlast;
            q.out_stride = C;
        }
    };
    {
        StreamBatchParams q = base(h->layers[0]);
        ring_in(q, 0);
        q.in_frame = m->frames;
        q.in_ring_w = m->rings + ring_off[0];
        q.in_clamp = look ? 1 : 0;
        out_to(q, 1);
        m->steps.push_back(q);
    }
    for (int b = 1; b <= nb; ++b) {
        StreamBatchParams k = base(h->layers[2 * b - 1]);
        ring_in(k, b);
        k.out = hbuf;
        k.out_stride = C;
        m->steps.push_back(k);
        StreamBatchParams pw = base(h->layers[2 * b]);
        plain_in(pw, hbuf);
        pw.res = m->rings + ring_off[b];
        pw.res_R = ring_len[b];
        pw.res_stride = (int64_t)ring_floats;
        // non-causal: the centre tap of the k-conv window (TemporalModel.py:132, causal_shift = 0);
        // ring b holds (taps - 1) dil + 1 >= 2 pad_b + 1 slots
        pw.res_back = look ? h->pad[b] : 0;
        out_to(pw, b + 1);
        m->steps.push_back(pw);
    }
    {
        StreamBatchParams q = base(h->layers[nl - 1]);
        plain_in(q, xlast);
        q.out = m->poses;
        q.out_stride = nout;
        q.out_gate = m->lookahead;
        m->steps.push_back(q);
    }
    hipDeviceSynchronize();  // setup memsets (legacy stream) before any launch on another stream
    *out = m;
    return VP3D_OK;
}

int mstream_capture(vp3d_mstream* m, void* stream) {
    if (!stream) return fail(VP3D_ERR_ARG, "graph capture needs a non-default stream");
    hipStream_t s = (hipStream_t)stream;
    if (m->exec) {
        hipGraphExecDestroy(m->exec);
        m->exec = nullptr;
    }
    if (m->graph) {
        hipGraphDestroy(m->graph);
        m->graph = nullptr;
    }
    HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = mstream_launch(m, s);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(s, &g);
    if (rc) return rc;
    if (e != hipSuccess) return fail(VP3D_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    m->graph = g;
    HIP_TRY(hipGraphInstantiate(&m->exec, g, nullptr, nullptr, 0));
    return VP3D_OK;
}

}  // namespace

extern "C" {

int vp3d_mstream_create(vp3d_handle* h, int dtype, int n_streams, vp3d_mstream** out) {
    return mstream_build(h, dtype, n_streams, false, out);
}

int vp3d_mstream_io(vp3d_mstream* m, float** frames, int32_t** active, float** poses) {
    if (!m) return fail(VP3D_ERR_ARG, "mstream is NULL");
    if (frames) *frames = m->frames;
    if (active) *active = mstream_active(m);
    if (poses) *poses = m->poses;
    return VP3D_OK;
}

int vp3d_mstream_step(vp3d_mstream* m, const float* frames, const int32_t* active, float* poses, void* stream) {
    if (!m) return fail(VP3D_ERR_ARG, "mstream is NULL");
    hipStream_t s = (hipStream_t)stream;
    const size_t cin0 = m->h->layers[0].cin, nout = m->h->layers.back().cout;
    if (frames) HIP_TRY(hipMemcpyAsync(m->frames, frames, 4 * m->S * cin0, hipMemcpyDeviceToDevice, s));
    if (active)
        HIP_TRY(hipMemcpyAsync(mstream_active(m), active, 4 * (size_t)m->S, hipMemcpyDeviceToDevice, s));
    else if (frames)
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)mstream_active(m), 1, (size_t)m->S, s));
    int rc = mstream_launch(m, s);
    if (rc) return rc;
    if (poses) HIP_TRY(hipMemcpyAsync(poses, m->poses, 4 * m->S * nout, hipMemcpyDeviceToDevice, s));
    return VP3D_OK;
}

int vp3d_mstream_reset(vp3d_mstream* m, int slot, void* stream) {
    if (!m) return fail(VP3D_ERR_ARG, "mstream is NULL");
    if (slot < -1 || slot >= m->S) return fail(VP3D_ERR_ARG, "slot must be -1 or 0..n_streams-1");
    if (slot < 0)
        HIP_TRY(hipMemsetAsync(m->pos, 0, 4 * (size_t)m->S, (hipStream_t)stream));
    else
        HIP_TRY(hipMemsetAsync(m->pos + slot, 0, 4, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_mstream_frames_seen(vp3d_mstream* m, int64_t* out) {
    if (!m || !out) return fail(VP3D_ERR_ARG, "NULL argument");
    std::vector<int> t((size_t)m->S);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(t.data(), m->pos, 4 * (size_t)m->S, hipMemcpyDeviceToHost));
    for (int s = 0; s < m->S; ++s) out[s] = t[s];
    return VP3D_OK;
}

int vp3d_mstream_graph_capture(vp3d_mstream* m, void* stream) {
    if (!m) return fail(VP3D_ERR_ARG, "mstream is NULL");
    return mstream_capture(m, stream);
}

int vp3d_mstream_graph_launch(vp3d_mstream* m, void* stream) {
    if (!m || !m->exec) return fail(VP3D_ERR_STATE, "no captured graph");
    HIP_TRY(hipGraphLaunch(m->exec, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_mstream_destroy(vp3d_mstream* m) {
    if (!m) return VP3D_OK;
    mstream_free(m);
    return VP3D_OK;
}

// ---- look-ahead streaming of non-causal models (stream_batch.hip, look-ahead form) ----

int vp3d_lstream_create(vp3d_handle* h, int dtype, int n_streams, vp3d_lstream** out) {
    if (!h || !out) return fail(VP3D_ERR_ARG, "NULL argument");
    *out = nullptr;
    vp3d_mstream* m = nullptr;
    int rc = mstream_build(h, dtype, n_streams, true, &m);
    if (rc) return rc;
    vp3d_lstream* l = new vp3d_lstream();
    l->m = m;
    *out = l;
    return VP3D_OK;
}

int vp3d_lstream_lookahead(vp3d_lstream* l, int32_t* out) {
    if (!l || !out) return fail(VP3D_ERR_ARG, "NULL argument");
    *out = l->m->lookahead;
    return VP3D_OK;
}

int vp3d_lstream_io(vp3d_lstream* l, float** frames, int32_t** codes, float** poses, int32_t** pose_frame) {
    if (!l) return fail(VP3D_ERR_ARG, "lstream is NULL");
    if (frames) *frames = l->m->frames;
    if (codes) *codes = mstream_active(l->m);
    if (poses) *poses = l->m->poses;
    if (pose_frame) *pose_frame = mstream_pose_frame(l->m);
    return VP3D_OK;
}

int vp3d_lstream_step(vp3d_lstream* l, const float* frames, const int32_t* codes, float* poses, int32_t* pose_frame,
                      void* stream) {
    if (!l) return fail(VP3D_ERR_ARG, "lstream is NULL");
    vp3d_mstream* m = l->m;
    hipStream_t s = (hipStream_t)stream;
    const size_t cin0 = m->h->layers[0].cin, nout = m->h->layers.back().cout;
    if (frames) HIP_TRY(hipMemcpyAsync(m->frames, frames, 4 * m->S * cin0, hipMemcpyDeviceToDevice, s));
    if (codes)
        HIP_TRY(hipMemcpyAsync(mstream_active(m), codes, 4 * (size_t)m->S, hipMemcpyDeviceToDevice, s));
    else if (frames)
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)mstream_active(m), kStreamCodeConsume, (size_t)m->S, s));
    int rc = mstream_launch(m, s);
    if (rc) return rc;
    if (poses) HIP_TRY(hipMemcpyAsync(poses, m->poses, 4 * m->S * nout, hipMemcpyDeviceToDevice, s));
    if (pose_frame)
        HIP_TRY(hipMemcpyAsync(pose_frame, mstream_pose_frame(m), 4 * (size_t)m->S, hipMemcpyDeviceToDevice, s));
    return VP3D_OK;
}

int vp3d_lstream_reset(vp3d_lstream* l, int slot, void* stream) {
    if (!l) return fail(VP3D_ERR_ARG, "lstream is NULL");
    vp3d_mstream* m = l->m;
    if (slot < -1 || slot >= m->S) return fail(VP3D_ERR_ARG, "slot must be -1 or 0..n_streams-1");
    // steps taken and frames consumed; the poses emitted and the drained state follow from them
    const size_t first = slot < 0 ? 0 : (size_t)slot, bytes = slot < 0 ? 4 * (size_t)m->S : 4;
    HIP_TRY(hipMemsetAsync(m->pos + first, 0, bytes, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(mstream_consumed(m) + first, 0, bytes, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_lstream_counts(vp3d_lstream* l, int64_t* consumed, int64_t* emitted) {
    if (!l || (!consumed && !emitted)) return fail(VP3D_ERR_ARG, "NULL argument");
    vp3d_mstream* m = l->m;
    std::vector<int> tn(3 * (size_t)m->S);  // t, codes (unused), n
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(tn.data(), m->pos, 12 * (size_t)m->S, hipMemcpyDeviceToHost));
    for (int s = 0; s < m->S; ++s) {
        const int t = tn[s], n = tn[2 * (size_t)m->S + s];
        if (consumed) consumed[s] = n;
        if (emitted) emitted[s] = t > m->lookahead ? t - m->lookahead : 0;
    }
    return VP3D_OK;
}

int vp3d_lstream_graph_capture(vp3d_lstream* l, void* stream) {
    if (!l) return fail(VP3D_ERR_ARG, "lstream is NULL");
    return mstream_capture(l->m, stream);
}

int vp3d_lstream_graph_launch(vp3d_lstream* l, void* stream) {
    if (!l || !l->m->exec) return fail(VP3D_ERR_STATE, "no captured graph");
    HIP_TRY(hipGraphLaunch(l->m->exec, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_lstream_destroy(vp3d_lstream* l) {
    if (!l) return VP3D_OK;
    mstream_free(l->m);
    delete l;
    return VP3D_OK;
}

// ---- on-device input path ----

int vp3d_normalize_screen(const float* x, int64_t n_points, int32_t w, int32_t h, float* out,
                          void* stream) {
    if (n_points < 0 || (n_points > 0 && (!x || !out))) return fail(VP3D_ERR_ARG, "bad pointer");
    if (w <= 0) return fail(VP3D_ERR_ARG, "w must be positive");
    HIP_TRY(launch_normalize_screen(x, n_points, w, h, out, false, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_normalize_screen_f64(const double* x, int64_t n_points, double w, double hw, float* out, void* stream) {
    if (!x || !out) return fail(VP3D_ERR_ARG, "x / out is NULL");
    if (!(w > 0.0)) return fail(VP3D_ERR_ARG, "w must be positive");
    HIP_TRY(launch_normalize_screen_f64(x, n_points, w, hw, out, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_image_coordinates(const float* x, int64_t n_points, int32_t w, int32_t h, float* out,
                           void* stream) {
    if (n_points < 0 || (n_points > 0 && (!x || !out))) return fail(VP3D_ERR_ARG, "bad pointer");
    if (w <= 0) return fail(VP3D_ERR_ARG, "w must be positive");
    HIP_TRY(launch_normalize_screen(x, n_points, w, h, out, true, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_camera_matrices(const float* intr, const int32_t* frame_seq, const double* extr,
                         int64_t n_frames, float* out, void* stream) {
    if (n_frames < 0 || (n_frames > 0 && (!intr || !frame_seq || !extr || !out)))
        return fail(VP3D_ERR_ARG, "bad pointer");
    HIP_TRY(launch_camera_matrices(intr, frame_seq, extr, n_frames, out, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_world_to_camera(const float* X, int64_t n_points, const float* R_host, const float* t_host,
                         float* out, void* stream) {
    if (!R_host || !t_host) return fail(VP3D_ERR_ARG, "R / t is NULL");
    if (n_points < 0 || (n_points > 0 && (!X || !out))) return fail(VP3D_ERR_ARG, "bad pointer");
    HIP_TRY(launch_world_to_camera(X, n_points, R_host, t_host, out, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_gather_windows(const float* kps, int32_t f2, const float* cams, const int64_t* seq_off,
                        const int32_t* seq_len, const int32_t* pairs, int32_t B, int32_t window,
                        int32_t pad, int32_t causal_shift, float* out, void* stream) {
    if (B < 0 || window <= 0 || f2 <= 0) return fail(VP3D_ERR_ARG, "bad sizes");
    if (B > 0 && (!kps || !seq_off || !seq_len || !pairs || !out)) return fail(VP3D_ERR_ARG, "bad pointer");
    HIP_TRY(launch_gather_windows(kps, f2, cams, seq_off, seq_len, pairs, B, window, pad,
                                  causal_shift, out, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_mpjpe_accumulate(const float* pred, const float* target, int64_t n_points, double* acc,
                          void* stream) {
    if (n_points < 0 || (n_points > 0 && (!pred || !target || !acc)))
        return fail(VP3D_ERR_ARG, "bad pointer");
    HIP_TRY(launch_mpjpe_accumulate(pred, target, n_points, acc, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_mpjpe_backward(const float* pred, const float* target, int64_t n_points, const float* grad_loss,
                        float* grad_pred, void* stream) {
    if (n_points < 0 || (n_points > 0 && (!pred || !target || !grad_loss || !grad_pred)))
        return fail(VP3D_ERR_ARG, "bad pointer");
    HIP_TRY(launch_mpjpe_backward(pred, target, n_points, grad_loss, grad_pred, (hipStream_t)stream));
    return VP3D_OK;
}


int vp3d_project_to_2d(const float* X, int64_t n_cams, int64_t pts_per_cam, const float* params, int32_t linear,
                       float* out, void* stream) {
    if (n_cams < 0 || pts_per_cam < 0) return fail(VP3D_ERR_ASSERT, "shape mismatch");
    if (n_cams * pts_per_cam > 0 && (!X || !params || !out)) return fail(VP3D_ERR_ARG, "bad pointer");
    HIP_TRY(launch_project_to_2d(X, n_cams, pts_per_cam, params, linear != 0, out, (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_pose_metrics(const float* pred, const float* target, int64_t n_frames, int32_t n_joints, double* acc,
                      void* stream) {
    if (n_frames < 0 || n_joints <= 0) return fail(VP3D_ERR_ASSERT, "shape mismatch");
    if (!acc || (n_frames > 0 && (!pred || !target))) return fail(VP3D_ERR_ARG, "pred / target / acc is NULL");
    hipError_t e = launch_pose_metrics(pred, target, n_frames, n_joints, acc, (hipStream_t)stream);
    if (e != hipSuccess) return fail(VP3D_ERR_HIP, std::string("pose_metrics: ") + hipGetErrorString(e));
    return VP3D_OK;
}

}  // extern "C"
