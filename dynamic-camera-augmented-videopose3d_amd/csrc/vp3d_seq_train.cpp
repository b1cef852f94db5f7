// C-ABI of the CoupledLSTM training step (include/vp3d.h, "CoupledLSTM training step"): the
// train-mode forward and the backward of CoupledLSTM (reference common/models/CamLSTM.py:47-129
// in train mode, driven by run.py:451-487 with optim.Adam(amsgrad=True), run.py:662).
//
//   forward   [flat 2D | flat K.E] rows (CamLSTM.py:115-121) -> layer 0's gate pre-activations
//             on the f32 conv GEMM -> the recurrence (seq_train.hip lstm_train_fwd_kernel: gates,
//             cell and hidden states stored, nn.LSTM's inter-layer dropout) -> bn_lstm on batch
//             statistics -> per head layer Linear, BatchNorm1d (batch statistics, running-stat
//             update), LeakyReLU(0.01), Dropout -> the last Linear
//   backward  the head top down, bn_lstm, the backward through time (lstm_bptt_kernel: the gate
//             gradients da overwrite the stored gates), then per cell dW_ih = da^T x,
//             dW_hh = da^T h(t-1) on the split weight-gradient GEMM (train.hip launch_wgrad) and
//             db_ih = db_hh = colsum(da) (launch_colsum)
//
// The parameters are the module's own tensors, passed by device pointer on every call, so the
// transposed / packed forms the kernels read are rebuilt per forward.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dropout_hash.h"
#include "host.h"
#include "kernels.h"

using namespace vp3d;
using namespace vp3d::host;

namespace {

constexpr int64_t kSeqWgradPartFloats = 16ll << 20;  // 64 MB of split-row partials at most
constexpr float kLeakySlope = 0.01f;                  // nn.LeakyReLU() default (CamLSTM.py:90)

int pad_to(int v, int m) { return (v + m - 1) / m * m; }
size_t r4(size_t n) { return (n + 3) & ~(size_t)3; }

enum { kRoleRec = 0, kRoleBptt = 1, kRoleWgrad = 2, kRoleRest = 3 };

}  // namespace

struct vp3d_seq_trainer {
    vp3d_seq_cfg cfg{};
    int device = 0;
    int cin = 0, nout = 0, maxw = 0, nbn = 0;
    // per-step forms of the parameters
    float* wpack0 = nullptr;  // W_ih[0] as the conv GEMM's [Np][Kp]
    int Kp0 = 0, Np0 = 0;
    float* wih_t[4] = {nullptr, nullptr, nullptr, nullptr};
    float* whh_t[4] = {nullptr, nullptr, nullptr, nullptr};
    float* bias[4] = {nullptr, nullptr, nullptr, nullptr};
    float* ones = nullptr;
    float* bn = nullptr;  // per BatchNorm: mean, invstd, alpha, shift (maxw each)
    // (B, T)-sized arena
    char* arena = nullptr;
    size_t arena_bytes = 0;
    float *X = nullptr, *Gin = nullptr, *gates = nullptr, *cs = nullptr, *hs = nullptr, *xd = nullptr;
    float *hlast = nullptr, *dhlast = nullptr, *g[2] = {nullptr, nullptr}, *dz = nullptr, *coef = nullptr;
    float *dbias = nullptr, *wpart = nullptr;
    std::vector<float*> A, Z;  // A[0] = bn_lstm output, A[j+1] = head layer j's output; Z[j] its pre-BN rows
    double* red = nullptr;
    int64_t wpart_floats = 0;
    // latest forward
    bool have_fwd = false;
    int B = 0, T = 0;
    float p = 0.f;
    uint64_t seed = 0;
    // vp3d_seq_train_profile
    bool prof = false;
    std::vector<hipEvent_t> ev_a[4], ev_b[4];
};

namespace {

int check_device(const vp3d_seq_trainer* t) {
    int dev = 0;
    hipGetDevice(&dev);
    if (dev != t->device) return fail(VP3D_ERR_STATE, "trainer belongs to another device");
    return VP3D_OK;
}

float* bn_arr(vp3d_seq_trainer* t, int i, int which) { return t->bn + ((size_t)i * 4 + which) * t->maxw; }

void role_mark(vp3d_seq_trainer* t, int role, bool end, hipStream_t s) {
    if (!t->prof) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    hipEventRecord(e, s);
    (end ? t->ev_b : t->ev_a)[role].push_back(e);
}

void role_clear(vp3d_seq_trainer* t) {
    for (int r = 0; r < 4; ++r) {
        for (hipEvent_t e : t->ev_a[r]) hipEventDestroy(e);
        for (hipEvent_t e : t->ev_b[r]) hipEventDestroy(e);
        t->ev_a[r].clear();
        t->ev_b[r].clear();
    }
}

// param-table indices (vp3d_seq_weight_count order)
int idx_cell(int l) { return 4 * l; }                                          // weight_ih, weight_hh, bias_ih, bias_hh
int idx_bn_lstm(const vp3d_seq_cfg& c) { return 4 * c.num_layers; }            // weight, bias, running_mean, running_var
int idx_head(const vp3d_seq_cfg& c, int j) { return 4 * c.num_layers + 4 + 6 * j; }  // Linear w, b, BN w, b, rm, rv
int idx_last(const vp3d_seq_cfg& c) { return idx_head(c, c.n_head_layers); }

int head_in(const vp3d_seq_cfg& c, int j) { return j == 0 ? c.d_model : c.head_layers[j - 1]; }

int reserve(vp3d_seq_trainer* t, int B, int T) {
    const vp3d_seq_cfg& c = t->cfg;
    const int H = c.d_model, L = c.num_layers, n = c.n_head_layers;
    const size_t BT = (size_t)B * T;
    size_t f = 0;
    auto take = [&](size_t floats) {
        const size_t at = f;
        f += r4(floats);
        return at;
    };
    const size_t oX = take(BT * t->cin), oGin = take(BT * 4 * H), oGates = take((size_t)L * BT * 4 * H);
    const size_t oCs = take((size_t)L * B * (T + 1) * H), oHs = take((size_t)L * B * (T + 1) * H);
    const size_t oXd = take(L > 1 ? BT * H : 0);
    const size_t oHlast = take((size_t)B * H), oDhlast = take((size_t)B * H);
    std::vector<size_t> oA(n + 1), oZ(n);
    oA[0] = take((size_t)B * H);
    for (int j = 0; j < n; ++j) {
        oZ[j] = take((size_t)B * c.head_layers[j]);
        oA[j + 1] = take((size_t)B * c.head_layers[j]);
    }
    const size_t oG0 = take((size_t)B * t->maxw), oG1 = take((size_t)B * t->maxw), oDz = take((size_t)B * t->maxw);
    const size_t oCoef = take(3 * (size_t)t->maxw), oDbias = take(4 * (size_t)H);
    const int64_t max_nk = std::max<int64_t>((int64_t)4 * H * std::max(H, t->cin), (int64_t)t->maxw * t->maxw);
    const int64_t wpart_floats = std::max<int64_t>(kSeqWgradPartFloats, max_nk);
    const size_t oWpart = take((size_t)wpart_floats);
    int64_t red = std::max(train_reduce_part_doubles((int64_t)BT, 4 * H), train_reduce_part_doubles(B, H));
    red = std::max(red, train_reduce_part_doubles(B, t->nout));
    for (int j = 0; j < n; ++j) red = std::max(red, train_reduce_part_doubles(B, c.head_layers[j]));
    const size_t oRed = take(2 * (size_t)red);  // doubles; every offset is a multiple of 16 bytes
    const size_t bytes = f * sizeof(float);
    if (bytes > t->arena_bytes) {
        if (t->arena) HIP_TRY(hipFree(t->arena));
        t->arena = nullptr;
        t->arena_bytes = 0;
        if (hipMalloc(&t->arena, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(VP3D_ERR_OOM, "activation store of " + std::to_string(bytes) + " bytes for B = " +
                                          std::to_string(B) + ", T = " + std::to_string(T) +
                                          " could not be allocated");
        }
        t->arena_bytes = bytes;
    }
    float* a = (float*)t->arena;
    t->X = a + oX;
    t->Gin = a + oGin;
    t->gates = a + oGates;
    t->cs = a + oCs;
    t->hs = a + oHs;
    t->xd = a + oXd;
    t->hlast = a + oHlast;
    t->dhlast = a + oDhlast;
    t->A.assign(n + 1, nullptr);
    t->Z.assign(n, nullptr);
    for (int j = 0; j <= n; ++j) t->A[j] = a + oA[j];
    for (int j = 0; j < n; ++j) t->Z[j] = a + oZ[j];
    t->g[0] = a + oG0;
    t->g[1] = a + oG1;
    t->dz = a + oDz;
    t->coef = a + oCoef;
    t->dbias = a + oDbias;
    t->wpart = a + oWpart;
    t->wpart_floats = wpart_floats;
    t->red = (double*)(a + oRed);
    return VP3D_OK;
}

// dW (torch layout [N][K]) = dZ^T X over M rows; dZ row of (b, t) = b*T_out + t, X row = b*T_in + t
// (mark: timed as a weight-gradient GEMM; the head's count with the head)
int wgrad(vp3d_seq_trainer* t, const float* dZ, int N, const float* X, int K, int64_t M, int T_out, int T_in,
          float* dW, hipStream_t s, bool mark = true) {
    WgradParams w{};
    w.dZ = dZ;
    w.ldz = N;
    w.dz_T = T_out;
    w.dz_off = 0;
    w.X = X;
    w.cin = K;
    w.T_in = T_in;
    w.stride = 1;
    w.dil = 1;
    w.T_out = T_out;
    w.M = M;
    w.N = N;
    w.K = K;
    w.part = t->wpart;
    if ((int64_t)N * K > t->wpart_floats)
        return fail(VP3D_ERR_STATE, "weight-gradient partial buffer smaller than one N x K split");
    const int S = wgrad_splits(M, N, K, t->wpart_floats);
    if (mark) role_mark(t, kRoleWgrad, false, s);
    HIP_TRY(launch_wgrad(w, S, 1, dW, s));
    if (mark) role_mark(t, kRoleWgrad, true, s);
    return VP3D_OK;
}

}  // namespace

extern "C" {

int64_t vp3d_seq_train_bytes(const vp3d_seq_cfg* cfg, int B, int T) {
    if (!cfg || cfg->kind != VP3D_SEQ_LSTM || vp3d_seq_weight_count(cfg) < 0 || B <= 0 || T <= 0) return -1;
    return (int64_t)B * T * cfg->num_layers * 6 * cfg->d_model * 4;
}

int vp3d_seq_trainer_create(const vp3d_seq_cfg* cfg, vp3d_seq_trainer** out) {
    if (!out) return fail(VP3D_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!cfg) return fail(VP3D_ERR_ARG, "cfg is NULL");
    if (cfg->kind != VP3D_SEQ_LSTM)
        return fail(VP3D_ERR_ARG, "the sequence trainer trains VP3D_SEQ_LSTM only (the transformer's training is "
                                  "not on the MI355X path)");
    if (vp3d_seq_weight_count(cfg) < 0) return VP3D_ERR_ARG;  // message recorded by the validation
    vp3d_seq_trainer* t = new vp3d_seq_trainer();
    t->cfg = *cfg;
    if (t->cfg.eps <= 0.f) t->cfg.eps = 1e-5f;
    hipGetDevice(&t->device);
    const vp3d_seq_cfg& c = t->cfg;
    const int H = c.d_model, G = 4 * H;
    t->cin = c.num_joints_in * c.in_features + 12;
    t->nout = c.num_joints_out * c.out_features;
    t->maxw = std::max(G, t->nout);  // the BN / coefficient rows also serve as ones[4H]
    for (int j = 0; j < c.n_head_layers; ++j) t->maxw = std::max(t->maxw, c.head_layers[j]);
    t->nbn = 1 + c.n_head_layers;
    t->Np0 = pad_to(G, kPadN);
    t->Kp0 = pad_to(t->cin, kPadK);
    bool ok = hipMalloc(&t->wpack0, (size_t)t->Np0 * t->Kp0 * 4) == hipSuccess &&
              hipMemset(t->wpack0, 0, (size_t)t->Np0 * t->Kp0 * 4) == hipSuccess;
    for (int l = 0; ok && l < c.num_layers; ++l) {
        ok = hipMalloc(&t->whh_t[l], (size_t)H * G * 4) == hipSuccess &&
             hipMalloc(&t->bias[l], (size_t)G * 4) == hipSuccess;
        if (ok && l > 0) ok = hipMalloc(&t->wih_t[l], (size_t)H * G * 4) == hipSuccess;
    }
    std::vector<float> one(G, 1.0f);
    ok = ok && hipMalloc(&t->ones, (size_t)G * 4) == hipSuccess &&
         hipMemcpy(t->ones, one.data(), (size_t)G * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMalloc(&t->bn, (size_t)t->nbn * 4 * t->maxw * 4) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        vp3d_seq_trainer_destroy(t);
        return fail(VP3D_ERR_OOM, "sequence trainer constants");
    }
    *out = t;
    return VP3D_OK;
}

int vp3d_seq_trainer_destroy(vp3d_seq_trainer* t) {
    if (!t) return VP3D_OK;
    int prev = 0;
    hipGetDevice(&prev);
    hipSetDevice(t->device);
    hipFree(t->wpack0);
    for (int l = 0; l < 4; ++l) {
        hipFree(t->wih_t[l]);
        hipFree(t->whh_t[l]);
        hipFree(t->bias[l]);
    }
    hipFree(t->ones);
    hipFree(t->bn);
    hipFree(t->arena);
    role_clear(t);
    hipSetDevice(prev);
    delete t;
    return VP3D_OK;
}

int vp3d_seq_train_forward(vp3d_seq_trainer* t, float* const* params, int n_params, const float* x2d,
                           const float* xcam, int B, int T, float dropout_p, const double* momenta, uint64_t seed,
                           float* y, void* stream) {
    if (!t) return fail(VP3D_ERR_ARG, "trainer is NULL");
    if (!params || !x2d || !xcam || !y || !momenta) return fail(VP3D_ERR_ARG, "NULL argument");
    const vp3d_seq_cfg& c = t->cfg;
    const int want = vp3d_seq_weight_count(&c);
    if (n_params != want) return fail(VP3D_ERR_ARG, "expected " + std::to_string(want) + " parameters");
    for (int i = 0; i < n_params; ++i)
        if (!params[i]) return fail(VP3D_ERR_ARG, "parameter " + std::to_string(i) + " is NULL");
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(VP3D_ERR_ARG, "dropout p must be in [0, 1)");
    if (B < 2) return fail(VP3D_ERR_ARG, "Expected more than 1 value per channel when training (B = " +
                                             std::to_string(B) + ")");
    if (T < 1) return fail(VP3D_ERR_ASSERT, "frames must be positive");
    if ((int64_t)B * (T + 1) >= ((int64_t)1 << 31) / 4) return fail(VP3D_ERR_ARG, "too many rows");
    int rc = check_device(t);
    if (rc) return rc;
    t->have_fwd = false;
    rc = reserve(t, B, T);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int H = c.d_model, G = 4 * H, L = c.num_layers, n = c.n_head_layers;
    const int M = B * T;

    // per-step forms of the parameters, the input rows and layer 0's gate pre-activations
    role_mark(t, kRoleRest, false, s);
    HIP_TRY(launch_pack_weights(params[idx_cell(0)], G, t->cin, 1, 0, t->Kp0, t->wpack0, s));
    for (int l = 0; l < L; ++l) {
        float* const* cp = params + idx_cell(l);
        if (l > 0) HIP_TRY(launch_pack_weights(cp[0], G, H, 1, 2, G, t->wih_t[l], s));
        HIP_TRY(launch_pack_weights(cp[1], G, H, 1, 2, G, t->whh_t[l], s));
        HIP_TRY(launch_vec_add(cp[2], cp[3], G, t->bias[l], s));
    }
    HIP_TRY(launch_concat_frames(x2d, t->cin - 12, xcam, 12, M, t->X, s));
    {
        ConvGemmParams p{};
        p.A = t->X;
        p.W = t->wpack0;
        p.scale = t->ones;
        p.shift = t->bias[0];
        p.Y = t->Gin;
        p.M = M;
        p.N = G;
        p.K = t->cin;
        p.Kp = t->Kp0;
        p.T_out = M;
        p.T_in = M;
        p.stride = 1;
        p.dil = 1;
        p.Ktap = t->cin;
        p.lda = t->cin;
        p.R_stride = 1;
        p.ldr = G;
        p.ldy = G;
        HIP_TRY(launch_conv_gemm(p, Act::F32, Act::F32, Act::F32, s));
    }
    role_mark(t, kRoleRest, true, s);

    LstmTrainParams lp{};
    lp.gin = t->Gin;
    lp.B = B;
    lp.T = T;
    lp.H = H;
    lp.L = L;
    for (int l = 0; l < L; ++l) {
        lp.wih_t[l] = t->wih_t[l];
        lp.whh_t[l] = t->whh_t[l];
        lp.bias[l] = t->bias[l];
    }
    lp.gates = t->gates;
    lp.cs = t->cs;
    lp.hs = t->hs;
    lp.hlast = t->hlast;
    lp.dscale = keep_scale(dropout_p);
    lp.seed = seed;
    lp.thresh = keep_threshold(dropout_p);
    role_mark(t, kRoleRec, false, s);
    HIP_TRY(launch_lstm_train_fwd(lp, s));
    role_mark(t, kRoleRec, true, s);

    role_mark(t, kRoleRest, false, s);
    {
        float* const* bp = params + idx_bn_lstm(c);
        HIP_TRY(launch_bn_train_stats(t->hlast, B, H, t->red, bp[0], bp[1], c.eps, momenta[0], bp[2], bp[3],
                                      bn_arr(t, 0, 0), bn_arr(t, 0, 1), bn_arr(t, 0, 2), bn_arr(t, 0, 3), s));
        HIP_TRY(launch_bn_leaky_fwd(t->hlast, B, H, bn_arr(t, 0, 2), bn_arr(t, 0, 3), 1.0f, 0.f, seed, 0, t->A[0], s));
    }
    for (int j = 0; j < n; ++j) {
        float* const* hp = params + idx_head(c, j);
        const int K = head_in(c, j), N = c.head_layers[j];
        HIP_TRY(launch_head_linear(t->A[j], hp[0], hp[1], B, N, K, t->Z[j], s));
        HIP_TRY(launch_bn_train_stats(t->Z[j], B, N, t->red, hp[2], hp[3], c.eps, momenta[j + 1], hp[4], hp[5],
                                      bn_arr(t, j + 1, 0), bn_arr(t, j + 1, 1), bn_arr(t, j + 1, 2),
                                      bn_arr(t, j + 1, 3), s));
        HIP_TRY(launch_bn_leaky_fwd(t->Z[j], B, N, bn_arr(t, j + 1, 2), bn_arr(t, j + 1, 3), kLeakySlope, dropout_p,
                                    seed, L - 1 + j, t->A[j + 1], s));
    }
    {
        float* const* lp2 = params + idx_last(c);
        HIP_TRY(launch_head_linear(t->A[n], lp2[0], lp2[1], B, t->nout, head_in(c, n), y, s));
    }
    role_mark(t, kRoleRest, true, s);
    t->have_fwd = true;
    t->B = B;
    t->T = T;
    t->p = dropout_p;
    t->seed = seed;
    return VP3D_OK;
}

int vp3d_seq_train_backward(vp3d_seq_trainer* t, float* const* params, int n_params, const float* dy,
                            float* const* grads, void* stream) {
    if (!t) return fail(VP3D_ERR_ARG, "trainer is NULL");
    if (!t->have_fwd) return fail(VP3D_ERR_STATE, "vp3d_seq_train_backward without a preceding forward");
    if (!params || !dy || !grads) return fail(VP3D_ERR_ARG, "NULL argument");
    const vp3d_seq_cfg& c = t->cfg;
    if (n_params != vp3d_seq_weight_count(&c)) return fail(VP3D_ERR_ARG, "parameter count mismatch");
    for (int i = 0; i < n_params; ++i)
        if (!params[i]) return fail(VP3D_ERR_ARG, "parameter " + std::to_string(i) + " is NULL");
    int rc = check_device(t);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int H = c.d_model, G = 4 * H, L = c.num_layers, n = c.n_head_layers;
    const int B = t->B, T = t->T;
    const int64_t M = (int64_t)B * T;
    t->have_fwd = false;  // the backward through time overwrites the stored gates

    // the head, top down: g[cur] = gradient wrt A[j + 1]
    role_mark(t, kRoleRest, false, s);
    int cur = 0;
    {
        const int il = idx_last(c), K = head_in(c, n);
        if (grads[il + 1]) HIP_TRY(launch_colsum(dy, B, t->nout, t->nout, t->red, grads[il + 1], s));
        if (grads[il] && (rc = wgrad(t, dy, t->nout, t->A[n], K, B, B, B, grads[il], s, false))) return rc;
        HIP_TRY(launch_head_linear_dgrad(dy, params[il], B, t->nout, K, t->g[cur], s));
    }
    for (int j = n - 1; j >= 0; --j) {
        const int ih = idx_head(c, j), K = head_in(c, j), N = c.head_layers[j];
        HIP_TRY(launch_bn_leaky_bwd(t->g[cur], t->Z[j], B, N, params[ih + 2], bn_arr(t, j + 1, 2), bn_arr(t, j + 1, 3),
                                    bn_arr(t, j + 1, 0), bn_arr(t, j + 1, 1), kLeakySlope, t->p, t->seed, L - 1 + j,
                                    t->coef, grads[ih + 2], grads[ih + 3], t->dz, s));
        if (grads[ih + 1]) HIP_TRY(launch_colsum(t->dz, B, N, N, t->red, grads[ih + 1], s));
        if (grads[ih] && (rc = wgrad(t, t->dz, N, t->A[j], K, B, B, B, grads[ih], s, false))) return rc;
        HIP_TRY(launch_head_linear_dgrad(t->dz, params[ih], B, N, K, t->g[cur ^ 1], s));
        cur ^= 1;
    }
    {
        const int ib = idx_bn_lstm(c);
        HIP_TRY(launch_bn_leaky_bwd(t->g[cur], t->hlast, B, H, params[ib], bn_arr(t, 0, 2), bn_arr(t, 0, 3),
                                    bn_arr(t, 0, 0), bn_arr(t, 0, 1), 1.0f, 0.f, t->seed, 0, t->coef, grads[ib],
                                    grads[ib + 1], t->dhlast, s));
    }
    role_mark(t, kRoleRest, true, s);

    LstmBpttParams bp{};
    bp.B = B;
    bp.T = T;
    bp.H = H;
    bp.L = L;
    for (int l = 0; l < L; ++l) {
        bp.wih[l] = l > 0 ? params[idx_cell(l)] : nullptr;
        bp.whh[l] = params[idx_cell(l) + 1];
    }
    bp.gates = t->gates;
    bp.cs = t->cs;
    bp.dhlast = t->dhlast;
    bp.dscale = keep_scale(t->p);
    bp.seed = t->seed;
    bp.thresh = keep_threshold(t->p);
    role_mark(t, kRoleBptt, false, s);
    HIP_TRY(launch_lstm_bptt(bp, s));
    role_mark(t, kRoleBptt, true, s);

    for (int l = 0; l < L; ++l) {
        const int ic = idx_cell(l);
        const float* da = t->gates + (size_t)l * M * G;
        if (grads[ic + 2] || grads[ic + 3]) {
            role_mark(t, kRoleWgrad, false, s);
            HIP_TRY(launch_colsum(da, M, G, G, t->red, t->dbias, s));
            for (int k = 2; k < 4; ++k)
                if (grads[ic + k])
                    HIP_TRY(hipMemcpyAsync(grads[ic + k], t->dbias, (size_t)G * 4, hipMemcpyDeviceToDevice, s));
            role_mark(t, kRoleWgrad, true, s);
        }
        if (grads[ic]) {
            if (l == 0) {
                if ((rc = wgrad(t, da, G, t->X, t->cin, M, T, T, grads[ic], s))) return rc;
            } else {
                role_mark(t, kRoleRest, false, s);
                HIP_TRY(launch_lstm_drop_rows(t->hs + (size_t)(l - 1) * B * (T + 1) * H, B, T, H, t->p, t->seed, l - 1,
                                              t->xd, s));
                role_mark(t, kRoleRest, true, s);
                if ((rc = wgrad(t, da, G, t->xd, H, M, T, T, grads[ic], s))) return rc;
            }
        }
        if (grads[ic + 1] &&
            (rc = wgrad(t, da, G, t->hs + (size_t)l * B * (T + 1) * H, H, M, T, T + 1, grads[ic + 1], s)))
            return rc;
    }
    return VP3D_OK;
}

int vp3d_seq_train_mask(vp3d_seq_trainer* t, int site, int which, int64_t n, uint8_t* out, void* stream) {
    if (!t || !out) return fail(VP3D_ERR_ARG, "NULL argument");
    if (t->B <= 0) return fail(VP3D_ERR_STATE, "no forward yet");
    const vp3d_seq_cfg& c = t->cfg;
    const int L = c.num_layers;
    if (site < 0 || site >= L - 1 + c.n_head_layers) return fail(VP3D_ERR_ARG, "site out of range");
    if (which != 0 && which != 1) return fail(VP3D_ERR_ARG, "which must be 0 (dropout) or 1 (LeakyReLU side)");
    const bool lstm = site < L - 1;
    const int j = site - (L - 1);
    const int64_t want = lstm ? (int64_t)t->B * t->T * c.d_model : (int64_t)t->B * c.head_layers[j];
    if (n != want) return fail(VP3D_ERR_ARG, "n must be " + std::to_string(want));
    int rc = check_device(t);
    if (rc) return rc;
    if (which == 0) {
        HIP_TRY(launch_dropout_mask(t->seed, t->p, site, n, out, (hipStream_t)stream));
        return VP3D_OK;
    }
    if (lstm) return fail(VP3D_ERR_ARG, "the LSTM dropout sites have no LeakyReLU");
    HIP_TRY(launch_relu_mask(t->Z[j], n, c.head_layers[j], bn_arr(t, j + 1, 2), bn_arr(t, j + 1, 3), out,
                             (hipStream_t)stream));
    return VP3D_OK;
}

int vp3d_seq_train_profile(vp3d_seq_trainer* t, int on, double* ms) {
    if (!t) return fail(VP3D_ERR_ARG, "trainer is NULL");
    int rc = check_device(t);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (ms) {
        for (int r = 0; r < 4; ++r) {
            ms[r] = 0.0;
            const size_t cnt = std::min(t->ev_a[r].size(), t->ev_b[r].size());
            for (size_t i = 0; i < cnt; ++i) {
                float v = 0.f;
                if (hipEventElapsedTime(&v, t->ev_a[r][i], t->ev_b[r][i]) == hipSuccess) ms[r] += v;
            }
        }
    }
    role_clear(t);
    t->prof = on != 0;
    return VP3D_OK;
}

}  // extern "C"
