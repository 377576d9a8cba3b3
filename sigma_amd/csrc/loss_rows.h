// loss_rows.h -- the row formulas of the option and focal losses, shared by the row kernels (pointwise.hip: a row of logits
// per thread) and the upsampled kernels (deepsup.hip: the interpolated row of a fine pixel).  The kinds, their formulas and
// why they are written the way they are: the comment above `enum Loss` in pointwise.hip.  Device helpers only, all forced
// inline; HAS_W = false: w = 1, W = C, no load.
#pragma once

#include <hip/hip_runtime.h>

namespace sigma {
namespace {

template <bool HAS_W>
__device__ __forceinline__ float ce_w(const float* __restrict__ w, int c) { return HAS_W ? w[c] : 1.0f; }

template <bool HAS_W>
__device__ __forceinline__ float ce_weight_sum(const float* __restrict__ w, int nc) {
    if (!HAS_W) return (float)nc;
    float W = 0.0f;
    for (int c = 0; c < nc; ++c) W += w[c];            // one fixed order for the forward and the backward
    return W;
}

// sum of w_c x_c over the n in [1, 4] valid columns of the chunk that starts at column c0 (columns past n are not touched:
// the pad may hold NaN and w ends at nc)
template <bool HAS_W>
__device__ __forceinline__ float ce_wx_chunk(const float* __restrict__ w, int c0, const float4& v, int n) {
    if (n >= 4) return (ce_w<HAS_W>(w, c0) * v.x + ce_w<HAS_W>(w, c0 + 1) * v.y) + (ce_w<HAS_W>(w, c0 + 2) * v.z + ce_w<HAS_W>(w, c0 + 3) * v.w);
    float t = ce_w<HAS_W>(w, c0) * v.x;
    if (n > 1) t += ce_w<HAS_W>(w, c0 + 1) * v.y;
    if (n > 2) t += ce_w<HAS_W>(w, c0 + 2) * v.z;
    return t;
}

// the option loss of a valid row (wy = w_y, W = sum of w, inv_c = 1 / C, sx = sum of w_c x_c)
__device__ __forceinline__ float ce_opt_row_loss(float eps, float inv_c, float wy, float W, float l, float xy, float sx) {
    float rl = ((1.0f - eps) * wy) * (l - xy);
    if (eps > 0.0f) rl += (eps * inv_c) * (W * l - sx);
    return rl;
}

// the option gradient of one chunk (fp, fa, fb = the three coefficients of the last line of the formula above); n as
// above: w is not read past it (what lands in columns >= n is overwritten by the caller)
template <bool HAS_W>
__device__ __forceinline__ float4 ce_opt_grad_chunk(const float* __restrict__ w, int c0, const float4& v, int n, float l, long y,
                                                    float fp, float fa, float fb) {
    float4 o;
    o.x = fp * __expf(v.x - l) - (y == c0 ? fa : 0.0f) - fb * ce_w<HAS_W>(w, c0);
    o.y = fp * __expf(v.y - l) - (y == c0 + 1 ? fa : 0.0f) - fb * (n > 1 ? ce_w<HAS_W>(w, c0 + 1) : 0.0f);
    o.z = fp * __expf(v.z - l) - (y == c0 + 2 ? fa : 0.0f) - fb * (n > 2 ? ce_w<HAS_W>(w, c0 + 2) : 0.0f);
    o.w = fp * __expf(v.w - l) - (y == c0 + 3 ? fa : 0.0f) - fb * (n > 3 ? ce_w<HAS_W>(w, c0 + 3) : 0.0f);
    return o;
}

// The focal factors of a valid row from xy = x_y and l = lse.  gamma = 2 is a square, gamma = 1 needs no power, anything
// else one exp(log) per row for t = q^(gamma - 1); q^gamma is t q throughout.  q = 0 (p_y rounds to 1): gamma > 0 gives
// loss 0 and m = 0 by a branch, never 0 * inf; gamma = 0 is the cross-entropy row (q^0 = 1, m = 1).  The forward and the
// backward form d, q and t with this code from the same lse.
struct FocalRow { float d, qg, m; };          // min(x_y - lse, 0), q^gamma and m

__device__ __forceinline__ FocalRow focal_row(float xy, float l, float gamma) {
    FocalRow f;
    const float d = f.d = fminf(xy - l, 0.0f);
    if (gamma == 0.0f) { f.qg = 1.0f; f.m = 1.0f; return f; }
    const float py = __expf(d);
    const float q = fmaxf(1.0f - py, 0.0f);
    if (!(q > 0.0f)) { f.qg = 0.0f; f.m = 0.0f; return f; }
    const float t = gamma == 2.0f ? q : gamma == 1.0f ? 1.0f : __expf((gamma - 1.0f) * __logf(q));
    f.qg = t * q;
    f.m = f.qg + ((gamma * t) * py) * (0.0f - d);
    return f;
}

}  // namespace
}  // namespace sigma
