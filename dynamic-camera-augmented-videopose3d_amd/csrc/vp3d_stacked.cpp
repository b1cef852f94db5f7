// C-ABI of the StackedPoseLifter ensemble MLP in eval mode (include/vp3d.h, "stacked pose
// lifter"): reference common/models/StackedPoseLifter.py:22-56, called per sequence at
// run.py:719-720.  The whole chain of Linears is one launch of stacked_lifter.hip; this file
// validates the configuration, packs the weights in the kernel's B-operand order and picks
// the row tile.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host.h"
#include "kernels.h"

using namespace vp3d;
using namespace vp3d::host;

struct vp3d_stacked {
    vp3d_stacked_cfg cfg{};
    int device = 0;
    int n_cu = 256;
    int mi_max = 1;  // largest row tile (16 mi rows) whose two activation buffers fit in LDS
    float* w = nullptr;
    StackedParams p{};
};

namespace {

int pad16(int v) { return (v + 15) / 16 * 16; }

int validate(const vp3d_stacked_cfg* c) {
    if (!c) return fail(VP3D_ERR_ARG, "cfg is NULL");
    if (c->num_joints <= 0 || c->features <= 0)
        return fail(VP3D_ERR_ASSERT, "num_joints and features must be positive");
    if (c->num_layers < 0 || c->num_layers > VP3D_STACKED_MAX_LAYERS)
        return fail(VP3D_ERR_ASSERT, "StackedPoseLifter: num_layers must be 0.." +
                                         std::to_string(VP3D_STACKED_MAX_LAYERS) + " (got " +
                                         std::to_string(c->num_layers) + ")");
    if (c->layer_size < 1 || c->layer_size > VP3D_STACKED_MAX_LAYER_SIZE)
        return fail(VP3D_ERR_ASSERT, "StackedPoseLifter: layer_size must be 1.." +
                                         std::to_string(VP3D_STACKED_MAX_LAYER_SIZE) + " (got " +
                                         std::to_string(c->layer_size) + ")");
    if ((int64_t)c->num_joints * c->features > VP3D_STACKED_MAX_POSE)
        return fail(VP3D_ERR_ASSERT, "StackedPoseLifter: num_joints * features must be at most " +
                                         std::to_string(VP3D_STACKED_MAX_POSE));
    return VP3D_OK;
}

int expected_weights(const vp3d_stacked_cfg* c) { return 2 * (c->num_layers + 2); }

// nn.Linear weight (N, K) -> [Np / 16][Kp / 16][64][4] (StackedParams), bias -> [Np]
void pack_linear(const float* W, const float* b, int N, int K, float* wdst, float* bdst) {
    const int Kp = pad16(K), Np = pad16(N), nk = Kp / 16;
    for (int jb = 0; jb < Np / 16; ++jb)
        for (int kt = 0; kt < nk; ++kt)
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 4; ++s) {
                    const int n = 16 * jb + (lane & 15), k = 16 * kt + 4 * (lane >> 4) + s;
                    wdst[(((size_t)jb * nk + kt) * 64 + lane) * 4 + s] = n < N && k < K ? W[(size_t)n * K + k] : 0.f;
                }
    for (int n = 0; n < Np; ++n) bdst[n] = n < N ? b[n] : 0.f;
}

}  // namespace

extern "C" {

int vp3d_stacked_weight_count(const vp3d_stacked_cfg* cfg) {
    if (validate(cfg)) return -1;
    return expected_weights(cfg);
}

int vp3d_stacked_create(const vp3d_stacked_cfg* cfg, const float* const* weights, int n_weights, vp3d_stacked** out) {
    if (!out) return fail(VP3D_ERR_ARG, "out is NULL");
    *out = nullptr;
    int rc = validate(cfg);
    if (rc) return rc;
    if (!weights || n_weights != expected_weights(cfg))
        return fail(VP3D_ERR_ARG, "expected " + std::to_string(expected_weights(cfg)) + " weight arrays");
    for (int i = 0; i < n_weights; ++i)
        if (!weights[i]) return fail(VP3D_ERR_ARG, "weight array " + std::to_string(i) + " is NULL");

    const int D = cfg->num_joints * cfg->features, H = cfg->layer_size;
    const int n_lin = cfg->num_layers + 2;
    StackedParams p{};
    p.D = D;
    p.n_lin = n_lin;
    size_t total = 0;
    int wmax = 0;
    for (int l = 0; l < n_lin; ++l) {
        const int K = l == 0 ? 2 * D : H, N = l + 1 == n_lin ? D : H;
        p.Kp[l] = pad16(K);
        p.Np[l] = pad16(N);
        p.w_off[l] = (int)total;
        total += (size_t)p.Kp[l] * p.Np[l];
        p.b_off[l] = (int)total;
        total += (size_t)p.Np[l];
        wmax = std::max(wmax, p.Kp[l]);  // the widest row an LDS buffer holds (a layer's input)
    }
    p.ld = wmax + 4;
    int mi_max = 0;
    for (int mi : {4, 2, 1})
        if (stacked_mlp_lds_bytes(mi, p.ld) <= kStackedMaxLds) {
            mi_max = mi;
            break;
        }
    if (!mi_max) return fail(VP3D_ERR_ASSERT, "StackedPoseLifter: 16 rows of the widest layer do not fit in LDS");

    std::vector<float> host(total);
    for (int l = 0; l < n_lin; ++l) {
        const int K = l == 0 ? 2 * D : H, N = l + 1 == n_lin ? D : H;
        pack_linear(weights[2 * l], weights[2 * l + 1], N, K, host.data() + p.w_off[l], host.data() + p.b_off[l]);
    }

    vp3d_stacked* h = new vp3d_stacked();
    h->cfg = *cfg;
    h->mi_max = mi_max;
    auto bail = [&](int code) {
        vp3d_stacked_destroy(h);
        return code;
    };
    hipError_t e = hipGetDevice(&h->device);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->device);
    if (e == hipSuccess) e = stacked_mlp_prepare();
    if (e == hipSuccess) e = hipMalloc(&h->w, total * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->w, host.data(), total * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess)
        return bail(fail(e == hipErrorOutOfMemory ? VP3D_ERR_OOM : VP3D_ERR_HIP,
                         std::string("vp3d_stacked_create: ") + hipGetErrorString(e)));
    p.w = h->w;
    h->p = p;
    *out = h;
    return VP3D_OK;
}

int vp3d_stacked_destroy(vp3d_stacked* h) {
    if (!h) return VP3D_OK;
    if (h->w) {
        int prev = 0;
        hipGetDevice(&prev);
        hipSetDevice(h->device);
        hipFree(h->w);
        hipSetDevice(prev);
    }
    delete h;
    return VP3D_OK;
}

int vp3d_stacked_forward(vp3d_stacked* h, const float* y_transformer, const float* y_fcn, int64_t n_rows, float* out,
                         void* stream) {
    if (!h || !y_transformer || !y_fcn || !out) return fail(VP3D_ERR_ARG, "NULL argument");
    if (n_rows <= 0) return fail(VP3D_ERR_ASSERT, "n_rows must be positive");
    if (n_rows > (int64_t)16 * 0x7FFFFFFF) return fail(VP3D_ERR_ARG, "too many rows");
    int dev = 0;
    hipGetDevice(&dev);
    if (dev != h->device) return fail(VP3D_ERR_STATE, "handle belongs to another device");
    // the largest row tile that fits, halved while the launch would leave CUs without a workgroup
    // (an output's summation order does not depend on the tile: stacked_lifter.hip)
    int mi = h->mi_max;
    while (mi > 1 && (n_rows + 16 * mi - 1) / (16 * mi) < h->n_cu) mi /= 2;
    StackedParams p = h->p;
    p.ya = y_transformer;
    p.yb = y_fcn;
    p.y = out;
    p.n_rows = n_rows;
    HIP_TRY(launch_stacked_mlp(p, mi, (hipStream_t)stream));
    return VP3D_OK;
}

}  // extern "C"
