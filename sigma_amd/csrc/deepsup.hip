// deepsup.hip -- bilinear x s upsampling fused with the loss of the deep-supervision heads: one forward and one backward
// kernel template for the plain mean cross entropy, the criteria with options and the focal loss (`enum UpLoss`).
//
// Reference: MambaDecoder.forward with deep_supervision (models/decoders/MambaDecoder.py:264-270) upsamples the normed
// decoder maps x16 / x8 / x4, runs a bias-free 1x1 convolution on the result and hands the full-size logits to
// nn.CrossEntropyLoss (models/builder.py:158-166).  The convolution acts on channels and the interpolation on space, so
// the two commute: the head runs on the COARSE tokens (sigma_amd/models/decoders/MambaDecoder.py) and the kernels here
// interpolate the `classes` logits of a fine pixel on the fly.  No full-size tensor is written or read; per head the
// traffic is the labels (8 bytes per fine pixel, twice), lse (4 bytes, written once and read once) and the coarse
// logits and their gradient, which stay in the caches.
//
//   upsample_loss_fwd one fine pixel per thread, rows in the order of softmax_ce_fwd_kernel (pointwise.hip) and its
//                     block_sum: lse of the interpolated row, the row's loss into the workgroup's (sum, weight) pair
//   upsample_loss_bwd GATHER: one group of lanes per (coarse pixel, chunk of 4 classes) walks the fine pixels of the coarse
//                     pixel's footprint in a fixed order (a lane per fine row, a fixed butterfly over the lanes), forms the
//                     interpolated chunk again from the 3 x 3 coarse neighbourhood it holds in registers and adds
//                     wgt d row_loss / d z (plain: wgt (exp(z - lse) - [c == y])); no atomics, every element of dlogits
//                     (pad included) is written by exactly one lane
//
// Index function of an axis with coarse size n and integer scale s (F.interpolate, align_corners=False):
//     src = max((dst + 0.5) / s - 0.5, 0) = max(num, 0) / (2 s),  num = 2 dst + 1 - s
//     i0 = floor(src), i1 = min(i0 + 1, n - 1), lambda = src - i0
// in integers, so i0 is exact for every s; lambda = rem / (2 s) is exact when s is a power of two.
// The interpolated logit:  R_k = fma(ly, v[i1][k], (1 - ly) v[i0][k]) for the two columns k, z = fma(lx, R_1, (1 - lx) R_0):
// four roundings on the way of any v, the same code in both directions.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ops_host.h"
#include "loss_rows.h"
#include "scan_device.h"

namespace sigma {
namespace {

constexpr float kNegInf = -INFINITY;

// lambda of a destination index whose lower tap i0 is known: rem = num - 2 s i0 (negative only left of the first sample)
__device__ __forceinline__ float tap_lambda(int num, int i0, int s2, float inv_s2) {
    const int rem = num - i0 * s2;
    return rem > 0 ? (float)rem * inv_s2 : 0.0f;
}

struct Tap { int i0, i1; float lam; };

__device__ __forceinline__ Tap tap(int dst, int s, int n, float inv_s2) {
    const int num = 2 * dst + 1 - s;
    Tap t;
    t.i0 = num > 0 ? num / (2 * s) : 0;
    t.i1 = min(t.i0 + 1, n - 1);
    t.lam = tap_lambda(num, t.i0, 2 * s, inv_s2);
    return t;
}

// the first destination index whose lower tap is >= k: i0(dst) >= k  <=>  dst >= s k + s / 2  (k >= 1)
__device__ __forceinline__ int tap_first(int k, int s) { return k >= 1 ? s * k + (s >> 1) : 0; }

__device__ __forceinline__ float lerp1(float lam, float a, float b) { return fmaf(lam, b, (1.0f - lam) * a); }

__device__ __forceinline__ float4 lerp4(float lam, const float4& a, const float4& b) {
    return make_float4(lerp1(lam, a.x, b.x), lerp1(lam, a.y, b.y), lerp1(lam, a.z, b.z), lerp1(lam, a.w, b.w));
}

__device__ __forceinline__ void mask_tail(float4& v, int n, float fill) {
    if (n < 2) v.y = fill;
    if (n < 3) v.z = fill;
    if (n < 4) v.w = fill;
}

__device__ __forceinline__ float4 sel4(bool c, const float4& a, const float4& b) {
    return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

// The criteria of the two kernels: the plain mean cross entropy (kUpPlain: no weights, no per-pixel loss or gradient; the
// pointers for them are NULL and never read), the criteria with options -- class weights, label smoothing, a per-pixel loss
// and upstream gradient (kUpOpt, the formulas of sigma_softmax_ce_opt_*) -- and the focal loss (kUpFocal,
// sigma_softmax_focal_*), applied to the interpolated row with the helpers of loss_rows.h.  The one float parameter `x` is
// eps for kUpOpt and gamma for kUpFocal, as in pointwise.hip.  HAS_W is false for kUpPlain.
enum UpLoss { kUpPlain, kUpOpt, kUpFocal };

// Forward.  Besides lse and the workgroup's pair: the row's loss (kUpOpt / kUpFocal, optional: 'none', and the nll the OHEM
// selection takes) and, for the focal loss, coef[P] = w_y m(P) -- the factor the backward puts beside the upstream
// gradient; its lanes hold one chunk of classes and cannot form z^_y themselves.
template <UpLoss KIND, bool HAS_W>
__global__ void __launch_bounds__(256)
upsample_loss_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ wt, int h,
                         int w, int s, int nc, int ld, long ignore, unsigned rows, float x, float* __restrict__ lse,
                         float* __restrict__ row_loss, float* __restrict__ coef, float* __restrict__ partial) {
    constexpr bool OPT = KIND == kUpOpt;
    __shared__ float sh[4];
    float loss = 0.0f, den = 0.0f;
    const unsigned W = (unsigned)(w * s), H = (unsigned)(h * s);
    const float inv_s2 = 1.0f / (float)(2 * s);
    const float Wsum = ce_weight_sum<OPT && HAS_W>(wt, nc), inv_c = 1.0f / (float)nc;        // kUpOpt only
    const unsigned stride = gridDim.x * blockDim.x;                     // 2^18: r + stride stays below 2^32
    for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const unsigned q = r / W, X = r - q * W, b = q / H, Y = q - b * H;
        const Tap ty = tap((int)Y, s, h, inv_s2), tx = tap((int)X, s, w, inv_s2);
        const float* __restrict__ p00 = logits + ((long)(b * h + ty.i0) * w + tx.i0) * ld;
        const float* __restrict__ p01 = logits + ((long)(b * h + ty.i0) * w + tx.i1) * ld;
        const float* __restrict__ p10 = logits + ((long)(b * h + ty.i1) * w + tx.i0) * ld;
        const float* __restrict__ p11 = logits + ((long)(b * h + ty.i1) * w + tx.i1) * ld;
        float m = kNegInf, sum = 0.0f, sx = 0.0f;                        // running max, sum of exp(z - m), sum of w_c z_c
        for (int c = 0; c < nc; c += 4) {
            const float4 v00 = *reinterpret_cast<const float4*>(p00 + c), v01 = *reinterpret_cast<const float4*>(p01 + c);
            const float4 v10 = *reinterpret_cast<const float4*>(p10 + c), v11 = *reinterpret_cast<const float4*>(p11 + c);
            float4 z = lerp4(tx.lam, lerp4(ty.lam, v00, v10), lerp4(ty.lam, v01, v11));
            if (OPT && x > 0.0f) sx += ce_wx_chunk<HAS_W>(wt, c, z, nc - c);
            mask_tail(z, nc - c, kNegInf);                               // the pad takes no part, whatever it holds
            const float zm = fmaxf(fmaxf(z.x, z.y), fmaxf(z.z, z.w));
            if (zm > m) { sum *= __expf(m - zm); m = zm; }
            sum += (__expf(z.x - m) + __expf(z.y - m)) + (__expf(z.z - m) + __expf(z.w - m));
        }
        const float l = m + __logf(sum);
        lse[r] = l;
        const long y = labels[r];
        float rl = 0.0f, cf = 0.0f;
        if (y != ignore && y >= 0 && y < nc) {
            const float wy = ce_w<HAS_W>(wt, (int)y);                    // 1 without weights: den counts the pixels
            const float zy = lerp1(tx.lam, lerp1(ty.lam, p00[y], p10[y]), lerp1(ty.lam, p01[y], p11[y]));
            if constexpr (KIND == kUpPlain) {
                rl = l - zy;
            } else if constexpr (OPT) {
                rl = ce_opt_row_loss(x, inv_c, wy, Wsum, l, zy, sx);
            } else {
                const FocalRow f = focal_row(zy, l, x);
                rl = wy * (f.qg * (0.0f - f.d));
                cf = wy * f.m;
            }
            loss += rl;
            den += wy;
        }
        if constexpr (KIND != kUpPlain) { if (row_loss) row_loss[r] = rl; }
        if constexpr (KIND == kUpFocal) coef[r] = cf;
    }
    const float tl = block_sum(loss, sh);
    const float td = block_sum(den, sh);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = tl; partial[2 * blockIdx.x + 1] = td; }
}

// One phase of the walk along x: the fine columns [xa, xb) all have the lower tap j0 (columns R0 | R1 of the
// row-interpolated neighbourhood); `own1` tells whether the coarse pixel is their upper tap (phase A: j0 = j - 1), else
// it is the lower one and, at the right border where both taps are clamped onto it, the upper one too.
// g_P = the upstream gradient of the fine pixel: sc (the device scalar) or its element of grad_row.  kUpOpt: the three
// coefficients of ce_opt_grad_chunk from y, w and g_P alone.  kUpFocal: the plain formula with g_P coef[P] in the place of
// g.  kUpPlain: g_P is one number for all pixels and is not applied here (see the kernel).
template <UpLoss KIND, bool HAS_W>
__device__ __forceinline__ void row_phase(int xa, int xb, int j0, bool own1, bool both, int s, float inv_s2, float wy,
                                          const float4& R0, const float4& R1, const int64_t* __restrict__ lab_row,
                                          const float* __restrict__ lse_row, const float* __restrict__ coef_row,
                                          const float* __restrict__ grad_row, float sc, const float* __restrict__ wt, float a1,
                                          float bW, float b, int c0, int nc, long ignore, float4& acc) {
    for (int X = xa; X < xb; ++X) {
        const long y = lab_row[X];
        if (!(y != ignore && y >= 0 && y < nc)) continue;
        const float lam = tap_lambda(2 * X + 1 - s, j0, 2 * s, inv_s2);
        const float wx = own1 ? lam : both ? (1.0f - lam) + lam : 1.0f - lam;
        const float wgt = wy * wx;
        const float l = lse_row[X];
        const float gp = grad_row ? grad_row[X] : sc;
        const float4 z = lerp4(lam, R0, R1);
        float4 o;
        if constexpr (KIND == kUpOpt) {
            const float a = a1 * ce_w<HAS_W>(wt, (int)y);
            o = ce_opt_grad_chunk<HAS_W>(wt, c0, z, nc - c0, l, y, gp * (a + bW), gp * a, gp * b);
        } else {
            o.x = __expf(z.x - l) - (y == c0 ? 1.0f : 0.0f);
            o.y = __expf(z.y - l) - (y == c0 + 1 ? 1.0f : 0.0f);
            o.z = __expf(z.z - l) - (y == c0 + 2 ? 1.0f : 0.0f);
            o.w = __expf(z.w - l) - (y == c0 + 3 ? 1.0f : 0.0f);
            if constexpr (KIND == kUpFocal) {
                const float g = gp * coef_row[X];
                o.x *= g; o.y *= g; o.z *= g; o.w *= g;
            }
        }
        acc.x = fmaf(wgt, o.x, acc.x);
        acc.y = fmaf(wgt, o.y, acc.y);
        acc.z = fmaf(wgt, o.z, acc.z);
        acc.w = fmaf(wgt, o.w, acc.w);
    }
}

// Backward.  A group of G lanes (a power of two <= 64: lanes of one wave) owns one (coarse pixel, chunk of 4 classes).  Lane k
// walks the fine rows ya + k, ya + k + G, ... of the footprint; the rows [ya, ym) have the lower tap i - 1 (the coarse pixel
// is their upper tap), the rows [ym, ye) the lower tap i.  The lanes' sums meet in a butterfly of fixed shape: same bits
// from run to run.  A thread alone per item (G = 1) walks (2 s)^2 fine pixels one dependent load after the other: at x16
// the 9600 coarse pixels of a 30 x 40 map do not fill the device and the kernel runs at the latency of a load (DESIGN.md
// 4.4), so the host picks G from the number of items.  The label's column is not gathered again.
// The upstream gradient: kUpOpt and kUpFocal apply g_P per fine pixel (it may differ from pixel to pixel: 'none').
// kUpPlain has the one scalar g = scale[0] and multiplies the finished sum by it, once per item: one multiply per element
// instead of one per fine pixel, and with -ffp-contract=off this order is what fixes the bits of the plain route.
template <UpLoss KIND, bool HAS_W>
__global__ void __launch_bounds__(256)
upsample_loss_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ lse,
                         const float* __restrict__ coef, const float* __restrict__ scale, const float* __restrict__ row_grad,
                         const float* __restrict__ wt, int h, int w, int s, int nc, int ld, long ignore, long items, int G, float x,
                         float* __restrict__ dlogits) {
    constexpr bool OPT = KIND == kUpOpt, PLAIN = KIND == kUpPlain;
    const int chunks = ld >> 2;
    const int H = h * s, W = w * s;
    const float inv_s2 = 1.0f / (float)(2 * s);
    const float sc = PLAIN || scale ? scale[0] : 0.0f;
    const float a1 = OPT ? 1.0f - x : 1.0f, b = OPT ? x * (1.0f / (float)nc) : 0.0f;
    const float bW = b * ce_weight_sum<OPT && HAS_W>(wt, nc);
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(tid & (G - 1));
    const long stride = ((long)gridDim.x * blockDim.x) / G;
    for (long t = tid / G; t < items; t += stride) {                     // the lanes of a group stay together
        const long px = t / chunks;                                      // coarse pixel (b, i, j), row of dlogits
        const int c0 = 4 * (int)(t - px * chunks);
        float4* __restrict__ out = reinterpret_cast<float4*>(dlogits + px * ld + c0);
        if (c0 >= nc) {
            if (lane == 0) *out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            continue;
        }
        const long bi = px / w;
        const int j = (int)(px - bi * w);
        const long bb = bi / h;
        const int i = (int)(bi - bb * h);
        // the 3 x 3 coarse neighbourhood of this chunk, indices clamped at the borders
        const int iu = max(i - 1, 0), id = min(i + 1, h - 1), jl = max(j - 1, 0), jr = min(j + 1, w - 1);
        const float* __restrict__ base = logits + bb * h * w * ld + c0;
        float4 Up[3], Mid[3], Dn[3];
        Up[0] = *reinterpret_cast<const float4*>(base + ((long)iu * w + jl) * ld);
        Up[1] = *reinterpret_cast<const float4*>(base + ((long)iu * w + j) * ld);
        Up[2] = *reinterpret_cast<const float4*>(base + ((long)iu * w + jr) * ld);
        Mid[0] = *reinterpret_cast<const float4*>(base + ((long)i * w + jl) * ld);
        Mid[1] = *reinterpret_cast<const float4*>(base + ((long)i * w + j) * ld);
        Mid[2] = *reinterpret_cast<const float4*>(base + ((long)i * w + jr) * ld);
        Dn[0] = *reinterpret_cast<const float4*>(base + ((long)id * w + jl) * ld);
        Dn[1] = *reinterpret_cast<const float4*>(base + ((long)id * w + j) * ld);
        Dn[2] = *reinterpret_cast<const float4*>(base + ((long)id * w + jr) * ld);
        const long img = bb * H * W;
        const int ya = tap_first(i - 1, s), ym = min(tap_first(i, s), H), ye = min(tap_first(i + 1, s), H);
        const int xa = tap_first(j - 1, s), xm = min(tap_first(j, s), W), xe = min(tap_first(j + 1, s), W);
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int Y = ya + lane; Y < ye; Y += G) {
            const bool up = Y < ym;                                      // lower tap i - 1: rows Up | Mid, else Mid | Dn
            const float lam = tap_lambda(2 * Y + 1 - s, up ? i - 1 : i, 2 * s, inv_s2);
            const float wy = up ? lam : i == h - 1 ? (1.0f - lam) + lam : 1.0f - lam;
            const float4 R0 = lerp4(lam, sel4(up, Up[0], Mid[0]), sel4(up, Mid[0], Dn[0]));
            const float4 R1 = lerp4(lam, sel4(up, Up[1], Mid[1]), sel4(up, Mid[1], Dn[1]));
            const float4 R2 = lerp4(lam, sel4(up, Up[2], Mid[2]), sel4(up, Mid[2], Dn[2]));
            const long row = img + (long)Y * W;
            const int64_t* __restrict__ lab_row = labels + row;
            const float* __restrict__ lse_row = lse + row;
            const float* __restrict__ coef_row = KIND == kUpFocal ? coef + row : nullptr;
            const float* __restrict__ grad_row = !PLAIN && row_grad ? row_grad + row : nullptr;
            row_phase<KIND, HAS_W>(xa, xm, j - 1, true, false, s, inv_s2, wy, R0, R1, lab_row, lse_row, coef_row, grad_row, sc, wt, a1,
                                   bW, b, c0, nc, ignore, acc);
            row_phase<KIND, HAS_W>(xm, xe, j, false, j == w - 1, s, inv_s2, wy, R1, R2, lab_row, lse_row, coef_row, grad_row, sc, wt, a1,
                                   bW, b, c0, nc, ignore, acc);
        }
        for (int o = G >> 1; o > 0; o >>= 1) {
            acc.x += __shfl_xor(acc.x, o); acc.y += __shfl_xor(acc.y, o);
            acc.z += __shfl_xor(acc.z, o); acc.w += __shfl_xor(acc.w, o);
        }
        if (lane == 0) {
            if constexpr (PLAIN) acc = make_float4(acc.x * sc, acc.y * sc, acc.z * sc, acc.w * sc);
            mask_tail(acc, nc - c0, 0.0f);                               // exact zeros in the pad, chosen by index
            *out = acc;
        }
    }
}

// what sigma_upsample_ce_* hand to the shared check and launchers: no weight, row_loss, coef or row_grad
sigma_upsample_loss_params up_plain(const sigma_upsample_ce_params& p) {
    sigma_upsample_loss_params q = {};
    q.batch = p.batch, q.height = p.height, q.width = p.width, q.scale = p.scale, q.classes = p.classes, q.ld = p.ld;
    q.ignore_index = p.ignore_index, q.logits = p.logits, q.labels = p.labels, q.lse = p.lse;
    q.partial = p.partial, q.scale_grad = p.scale_grad, q.dlogits = p.dlogits;
    return q;
}

// everything all four entry points refuse on the geometry and the three pointers of both directions, before any launch;
// *fine = the number of fine pixels
int upsample_check(const sigma_upsample_loss_params& p, int64_t* fine) {
    if (p.classes < 1 || p.classes > 64 || p.ld % 4 != 0 || p.ld < p.classes)
        return fail(SIGMA_OPS_ERR_ARG, "classes %d must be in [1, 64] and ld %d a multiple of 4, at least classes", p.classes, p.ld);
    if (p.scale < 1 || p.scale > 32 || p.batch <= 0 || p.height <= 0 || p.width <= 0)
        return fail(SIGMA_OPS_ERR_ARG, "scale %d must be in [1, 32] and batch %d, height %d, width %d positive", p.scale, p.batch, p.height, p.width);
    // three factors below 2^31 and one below 2^6: the products of the first two pairs fit in 64 bits, the last is tested by division
    const int64_t coarse = (int64_t)p.batch * p.height;
    if (coarse > 2147483647LL / p.width)
        return fail(SIGMA_OPS_ERR_ARG, "batch %d x height %d x width %d coarse pixels exceed 2^31 - 1", p.batch, p.height, p.width);
    const int64_t ss = (int64_t)p.scale * p.scale;
    if (coarse * p.width > 2147483647LL / ss)
        return fail(SIGMA_OPS_ERR_ARG, "batch %d x height %d x width %d x scale %d^2 fine pixels exceed 2^31 - 1", p.batch, p.height, p.width, p.scale);
    *fine = coarse * p.width * ss;
    if (!p.logits || !p.labels || !p.lse || !aligned(p.logits, 16) || !aligned(p.labels, 8) || !aligned(p.lse, 4))
        return fail(SIGMA_OPS_ERR_ARG, "logits, labels and lse must be non-NULL device pointers aligned to 16, 8 and 4 bytes");
    return SIGMA_OPS_OK;
}

// what sigma_upsample_loss_* refuse on top of that in both directions: what the option and focal row kernels refuse on eps
// and gamma, the kind and the optional pointers
int upsample_loss_check(const sigma_upsample_loss_params* p, int64_t* fine) {
    if (!p) return fail(SIGMA_OPS_ERR_ARG, "params is NULL");
    if (const int rc = upsample_check(*p, fine)) return rc;
    if (p->kind != SIGMA_UPSAMPLE_LOSS_OPTIONS && p->kind != SIGMA_UPSAMPLE_LOSS_FOCAL)
        return fail(SIGMA_OPS_ERR_ARG, "kind must be SIGMA_UPSAMPLE_LOSS_OPTIONS (0) or SIGMA_UPSAMPLE_LOSS_FOCAL (1) (got %d)", p->kind);
    if (!(p->label_smoothing >= 0.0f && p->label_smoothing <= 1.0f))
        return fail(SIGMA_OPS_ERR_ARG, "label_smoothing %g must be in [0, 1]", (double)p->label_smoothing);
    if (p->kind == SIGMA_UPSAMPLE_LOSS_FOCAL) {
        if (p->label_smoothing != 0.0f || !(p->gamma == 0.0f || (p->gamma >= 1.0f && p->gamma < INFINITY)))
            return fail(SIGMA_OPS_ERR_ARG, "the focal kind needs label_smoothing 0 (got %g) and gamma 0 or finite >= 1 (got %g)",
                        (double)p->label_smoothing, (double)p->gamma);
        if (!p->coef || !aligned(p->coef, 4)) return fail(SIGMA_OPS_ERR_ARG, "the focal kind needs coef, a non-NULL 4-byte aligned device pointer");
    }
    if (!aligned(p->weight, 4)) return fail(SIGMA_OPS_ERR_ARG, "weight must be 4-byte aligned");
    return SIGMA_OPS_OK;
}

template <UpLoss KIND>
int up_launch_fwd(const sigma_upsample_loss_params& p, int64_t fine, float x, void* stream) {
    if (!p.partial || !aligned(p.partial, 4) || !aligned(p.row_loss, 4))
        return fail(SIGMA_OPS_ERR_ARG, "partial must be non-NULL, partial and row_loss 4-byte aligned");
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(SIGMA_CE_BLOCKS), dim3(256), 0, static_cast<hipStream_t>(stream), p.logits, p.labels, p.weight,
                           (int)p.height, (int)p.width, (int)p.scale, (int)p.classes, (int)p.ld, (long)p.ignore_index, (unsigned)fine, x,
                           p.lse, p.row_loss, p.coef, p.partial);
    };
    if (KIND != kUpPlain && p.weight) launch(upsample_loss_fwd_kernel<KIND, KIND != kUpPlain>);
    else launch(upsample_loss_fwd_kernel<KIND, false>);
    return launched("upsample_loss_fwd_kernel");
}

template <UpLoss KIND>
int up_launch_bwd(const sigma_upsample_loss_params& p, float x, void* stream) {
    if ((p.scale_grad != nullptr) == (p.row_grad != nullptr))
        return fail(SIGMA_OPS_ERR_ARG, "exactly one of scale_grad (%p) and row_grad (%p) must be given", (const void*)p.scale_grad, (const void*)p.row_grad);
    if (!p.dlogits || !aligned(p.scale_grad, 4) || !aligned(p.row_grad, 4) || !aligned(p.dlogits, 16))
        return fail(SIGMA_OPS_ERR_ARG, "dlogits must be non-NULL and 16-byte aligned, scale_grad and row_grad 4-byte aligned");
    const long items = (long)p.batch * p.height * p.width * (p.ld / 4);
    // lanes per item: as many as fill the device (2^19 resident threads), never more than the 2 s rows of a footprint.  A
    // function of the shape alone, so the order of the sums is too.
    int G = 1;
    while (G < 2 * p.scale && items * G < (1L << 19)) G <<= 1;
    long blocks = (items * G + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), p.logits, p.labels, p.lse,
                           p.coef, p.scale_grad, p.row_grad, p.weight, (int)p.height, (int)p.width, (int)p.scale, (int)p.classes,
                           (int)p.ld, (long)p.ignore_index, items, G, x, p.dlogits);
    };
    if (KIND != kUpPlain && p.weight) launch(upsample_loss_bwd_kernel<KIND, KIND != kUpPlain>);
    else launch(upsample_loss_bwd_kernel<KIND, false>);
    return launched("upsample_loss_bwd_kernel");
}

}  // namespace
}  // namespace sigma

extern "C" {

int sigma_upsample_loss_fwd(const sigma_upsample_loss_params* p, void* stream) {
    int64_t fine = 0;
    if (const int rc = sigma::upsample_loss_check(p, &fine)) return rc;
    if (p->kind == SIGMA_UPSAMPLE_LOSS_FOCAL) return sigma::up_launch_fwd<sigma::kUpFocal>(*p, fine, p->gamma, stream);
    return sigma::up_launch_fwd<sigma::kUpOpt>(*p, fine, p->label_smoothing, stream);
}

int sigma_upsample_loss_bwd(const sigma_upsample_loss_params* p, void* stream) {
    int64_t fine = 0;
    if (const int rc = sigma::upsample_loss_check(p, &fine)) return rc;
    if (p->kind == SIGMA_UPSAMPLE_LOSS_FOCAL) return sigma::up_launch_bwd<sigma::kUpFocal>(*p, p->gamma, stream);
    return sigma::up_launch_bwd<sigma::kUpOpt>(*p, p->label_smoothing, stream);
}

int sigma_upsample_ce_fwd(const sigma_upsample_ce_params* p, void* stream) {
    if (!p) return sigma::fail(SIGMA_OPS_ERR_ARG, "params is NULL");
    const sigma_upsample_loss_params q = sigma::up_plain(*p);
    int64_t fine = 0;
    if (const int rc = sigma::upsample_check(q, &fine)) return rc;
    return sigma::up_launch_fwd<sigma::kUpPlain>(q, fine, 0.0f, stream);
}

int sigma_upsample_ce_bwd(const sigma_upsample_ce_params* p, void* stream) {
    if (!p) return sigma::fail(SIGMA_OPS_ERR_ARG, "params is NULL");
    const sigma_upsample_loss_params q = sigma::up_plain(*p);
    int64_t fine = 0;
    if (const int rc = sigma::upsample_check(q, &fine)) return rc;
    return sigma::up_launch_bwd<sigma::kUpPlain>(q, 0.0f, stream);
}

}  // extern "C"
