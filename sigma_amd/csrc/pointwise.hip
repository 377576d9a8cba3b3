// pointwise.hip -- the squeeze/excite gate of the decoder's conv branch and the segmentation loss as HBM streams.
//
// Reference: ChannelAttention (models/encoders/vmamba.py:1725-1741): y = x * sigmoid(fc(avgpool(x)) + fc(maxpool(x)))
// on (B, C, H, W) activations, 12 calls per step in the Mamba decoder (:1744-1757, :1800-1805); and the loss of
// models/builder.py:146-166, nn.CrossEntropyLoss(reduction='mean', ignore_index) on the (B, classes, H, W) logits.
// ATen runs the gate as two plane reductions + a broadcast multiply and mirrors it in backward with ~10 elementwise /
// reduce launches over the activation (AmaxBackward0, MeanBackward1, MulBackward0: 4.5 ms per step,
// profiles/r03_aten_tail_by_node.txt); the loss as a transposing copy of the channels-last logits + log_softmax + nll
// and their three backward kernels (2.3 ms per step on 8 x 40 x 480 x 640).  Here:
//
//   plane_pool      one pass over x: mean, max and the number of elements equal to the max of every (b, c) plane
//   plane_scale     y = x * s[plane]
//   plane_dot       sum over the plane of g * x                       (gradient of the gate's pre-sigmoid input)
//   plane_gate_bwd  dx = g * s + dmean / HW + (x == max ? dmax / count : 0)   (amax backward: ties share the gradient)
//   softmax_ce_fwd  per pixel (a row of `classes` contiguous logits): log-sum-exp (kept for the backward) and the row's
//                   loss; per-workgroup partial (sum, weight or count) in a fixed layout -> deterministic mean
//   softmax_ce_bwd  dlogit from the logits and the kept log-sum-exp, zero rows for ignored pixels
//                   One family for three kinds of loss (enum Loss): the plain mean cross entropy lse - logit[label]; every
//                   option of nn.CrossEntropyLoss (class weights, label smoothing, a per-row loss ('none') and a per-row
//                   upstream gradient: the sigma_softmax_ce_opt entry points); and the focal loss w_y (1 - p_y)^gamma
//                   (lse - x_y) of FocalLoss2d (utils/loss_opr.py:12-23: the sigma_softmax_focal entry points)
//
// All of them are bound by HBM: bytes per element 4 (pool), 8 (scale, dot), 12 (gate_bwd), 4 / 8 (loss fwd / bwd).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "ops_host.h"
#include "loss_rows.h"
#include "scan_device.h"

namespace sigma {
namespace {

constexpr float kNegInf = -INFINITY;

__device__ __forceinline__ float wave_max_all(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ void max_count(float v, float& m, float& c) {
    if (v > m) { m = v; c = 1.0f; }
    else if (v == m) c += 1.0f;
}

__global__ void __launch_bounds__(256)
plane_pool_kernel(const float* __restrict__ x, long hw, int vec, float* __restrict__ mean, float* __restrict__ mx, float* __restrict__ cnt) {
    __shared__ float sh[12];
    const long plane = blockIdx.x;
    const float* __restrict__ xp = x + plane * hw;
    float s = 0.0f, m = kNegInf, c = 0.0f;
    if (vec) {
        const long n4 = hw >> 2;
        for (long i = threadIdx.x; i < n4; i += blockDim.x) {
            const float4 v = reinterpret_cast<const float4*>(xp)[i];
            s += (v.x + v.y) + (v.z + v.w);
            max_count(v.x, m, c); max_count(v.y, m, c); max_count(v.z, m, c); max_count(v.w, m, c);
        }
    } else {
        for (long i = threadIdx.x; i < hw; i += blockDim.x) { const float v = xp[i]; s += v; max_count(v, m, c); }
    }
    // A NaN is the maximum of its plane, as torch.amax and the reference's AdaptiveMaxPool2d have it, and equals nothing
    // (count 0); the comparisons above and fmaxf drop it.  The thread's sum is NaN whenever it read one (or both
    // infinities): only then it looks at its elements again, so the pass above costs what it did.
    if (s != s) {
        bool nan = false;
        if (vec) {
            for (long i = threadIdx.x; i < (hw >> 2); i += blockDim.x) {
                const float4 v = reinterpret_cast<const float4*>(xp)[i];
                nan = nan || v.x != v.x || v.y != v.y || v.z != v.z || v.w != v.w;
            }
        } else {
            for (long i = threadIdx.x; i < hw; i += blockDim.x) nan = nan || xp[i] != xp[i];
        }
        if (nan) m = __builtin_nanf("");
    }
    const float wm = __any(m != m) ? __builtin_nanf("") : wave_max_all(m);
    c = wave_sum(m == wm ? c : 0.0f);
    s = wave_sum(s);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[w] = s; sh[4 + w] = wm; sh[8 + w] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float ts = 0.0f, tm = kNegInf, tc = 0.0f;
        for (int i = 0; i < 4; ++i) {
            ts += sh[i];
            if (sh[4 + i] > tm) { tm = sh[4 + i]; tc = sh[8 + i]; }
            else if (sh[4 + i] == tm) tc += sh[8 + i];
            else if (sh[4 + i] != sh[4 + i]) tm = sh[4 + i];
        }
        mean[plane] = ts / (float)hw;
        mx[plane] = tm;
        cnt[plane] = tm != tm ? 0.0f : tc;
    }
}

__global__ void __launch_bounds__(256)
plane_dot_kernel(const float* __restrict__ a, const float* __restrict__ b, long hw, int vec, float* __restrict__ out) {
    __shared__ float sh[4];
    const long plane = blockIdx.x;
    const float* __restrict__ ap = a + plane * hw;
    const float* __restrict__ bp = b + plane * hw;
    float s = 0.0f;
    if (vec) {
        const long n4 = hw >> 2;
        for (long i = threadIdx.x; i < n4; i += blockDim.x) {
            const float4 u = reinterpret_cast<const float4*>(ap)[i];
            const float4 v = reinterpret_cast<const float4*>(bp)[i];
            s += (u.x * v.x + u.y * v.y) + (u.z * v.z + u.w * v.w);
        }
    } else {
        for (long i = threadIdx.x; i < hw; i += blockDim.x) s += ap[i] * bp[i];
    }
    const float t = block_sum(s, sh);
    if (threadIdx.x == 0) out[plane] = t;
}

__global__ void __launch_bounds__(256)
plane_scale_kernel(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ out, long planes, long hw, int vec) {
    const long stride = (long)gridDim.x * blockDim.x;
    if (vec) {
        const long n4 = hw >> 2, total = planes * n4;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
            const float f = s[i / n4];
            float4 v = reinterpret_cast<const float4*>(x)[i];
            v.x *= f; v.y *= f; v.z *= f; v.w *= f;
            reinterpret_cast<float4*>(out)[i] = v;
        }
    } else {
        const long total = planes * hw;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) out[i] = x[i] * s[i / hw];
    }
}

struct GateBwdArgs {
    const float* g; const float* x; const float* s; const float* dmean; const float* dmax; const float* mx; const float* cnt;
    float* dx; long planes, hw; int vec;
};

__global__ void __launch_bounds__(256) plane_gate_bwd_kernel(const GateBwdArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    const float inv = 1.0f / (float)a.hw;
    if (a.vec) {
        const long n4 = a.hw >> 2, total = a.planes * n4;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
            const long p = i / n4;
            const float f = a.s[p], dm = a.dmean[p] * inv, m = a.mx[p], dx_ = a.dmax[p] / a.cnt[p];
            const float4 g = reinterpret_cast<const float4*>(a.g)[i];
            const float4 v = reinterpret_cast<const float4*>(a.x)[i];
            float4 o;
            o.x = g.x * f + dm + (v.x == m ? dx_ : 0.0f);
            o.y = g.y * f + dm + (v.y == m ? dx_ : 0.0f);
            o.z = g.z * f + dm + (v.z == m ? dx_ : 0.0f);
            o.w = g.w * f + dm + (v.w == m ? dx_ : 0.0f);
            reinterpret_cast<float4*>(a.dx)[i] = o;
        }
    } else {
        const long total = a.planes * a.hw;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
            const long p = i / a.hw;
            a.dx[i] = a.g[i] * a.s[p] + a.dmean[p] * inv + (a.x[i] == a.mx[p] ? a.dmax[p] / a.cnt[p] : 0.0f);
        }
    }
}

// ---- the segmentation losses over rows of `nc` logits at a pitch of `ld` floats (ld % 4 == 0, ld >= nc), one thread per row
// PAD = false: nc % 4 == 0 and ld == nc, the contiguous rows of sigma_softmax_ce_fwd / _bwd.  PAD = true (ld != nc):
// only columns < nc count.  The forward reads the last 16-byte chunk that holds a valid column whole and puts
// -inf over its tail, later chunks are not read; the backward writes exact zeros over [nc, ld), chosen by index (the pad
// of the input may hold NaN, and the GEMMs that read dlogits take whole rows of ld).
__device__ __forceinline__ void ce_mask_tail(float4& v, int n, float fill) {      // n in [1, 4] columns of v are valid
    if (n < 2) v.y = fill;
    if (n < 3) v.z = fill;
    if (n < 4) v.w = fill;
}

// One family of four kernels -- forward / backward, walking the row or holding it in registers -- for three kinds of loss.
// The row loop, the loads, the tail mask, the online max / sum, the test of the label, the zero fill of the pad, the
// block sums and the partial pair exist once; a kind is the formula of a row's loss and of its gradient:
//   kPlain  (sigma_softmax_ce_fwd / _bwd and their _ld forms; HAS_W = false alone) the mean cross entropy,
//             row_loss = lse - x_y        dlogit_c = (p_c - [c == y]) g
//           which reads none of w, row_loss, row_grad and the float parameter.
//   kOpt    (sigma_softmax_ce_opt_fwd / _bwd) the options of nn.CrossEntropyLoss: class weights w, label smoothing eps,
//           a per-row loss and a per-row upstream gradient,
//             row_loss = (1 - eps) w_y (lse - x_y) + (eps / C) (W lse - sum_c w_c x_c),   W = sum_c w_c
//             dlogit_c = g [ (1 - eps) w_y (p_c - [c == y]) + (eps / C) (W p_c - w_c) ]
//                      = (g ((1 - eps) w_y + (eps / C) W)) p_c - [c == y] g (1 - eps) w_y - (g eps / C) w_c
//   kFocal  (sigma_softmax_focal_fwd / _bwd) FocalLoss2d (utils/loss_opr.py:12-23), weights and the per-row loss and
//           gradient as kOpt, no smoothing.  With d = x_y - lse <= 0, nll = -d, p_y = exp(d), q = 1 - p_y and the exponent
//           gamma (0 or >= 1, a run-time float):
//             row_loss = w_y q^gamma nll
//             dlogit_c = g w_y m (p_c - [c == y]),     m = q^gamma + gamma q^(gamma - 1) p_y nll
//           i.e. the plain gradient with g w_y m in the place of g: m is formed per row from the row the kernel holds anyway.
// The kernels' one float parameter `x` is eps for kOpt and gamma for kFocal.  The formulas are kept apart where they
// round differently: the plain one is the option one at w = 1, eps = 0 in exact arithmetic alone -- (e - 1) f and
// f e - f round differently -- and every kind keeps its bits.  The parameter lists are those the plain kernels have always
// had, the option-only parameters last in the backward, and the backward kernels write the plain formula out instead of
// calling a helper: with either changed the compiler schedules the plain kernels differently (at 40 and 48 classes with
// more registers and fewer waves).  Every pointer is a __restrict__ kernel parameter of its own: as members of a struct
// passed by value they lose the qualifier, and the w[c] become vector loads inside the row loop.  w is read through the
// caches, not staged in LDS: w[c] in the unrolled loops has a wave-uniform index (scalar loads, hoisted out of the row
// loop where the registers allow), w[y] is one gather per row from a table of at most a few cache lines.
// HAS_W = false: w = 1, W = C, no load.
enum Loss { kPlain, kOpt, kFocal };

// ce_w, ce_weight_sum, ce_wx_chunk, ce_opt_row_loss and ce_opt_grad_chunk: loss_rows.h (shared with deepsup.hip)

// the label's logit out of a row held in registers (0 where y is no column of it: the caller tests the label).  One
// chunk's step is a macro, not a function: the plain and option forward take it inside their sum loop, and through a
// helper the compiler lays the one-chunk kernels out differently.
#define SIGMA_CE_PICK(v, c0, y, xy) \
    ((y) == (c0)) ? (v).x : ((y) == (c0) + 1) ? (v).y : ((y) == (c0) + 2) ? (v).z : ((y) == (c0) + 3) ? (v).w : (xy)

template <int NC4>
__device__ __forceinline__ float ce_pick(const float4 (&v)[NC4], long y) {
    float xy = 0.0f;
#pragma unroll
    for (int c = 0; c < NC4; ++c) xy = SIGMA_CE_PICK(v[c], 4 * c, y, xy);
    return xy;
}

// FocalRow and focal_row, the focal factors of a valid row: loss_rows.h

__device__ __forceinline__ float focal_row_loss(float wy, float xy, float l, float gamma) {
    const FocalRow f = focal_row(xy, l, gamma);
    return wy * (f.qg * (0.0f - f.d));
}

// g w_y m of a valid row, g = the row's upstream gradient: what the plain gradient formula takes in the place of g
__device__ __forceinline__ float focal_row_grad(const float* __restrict__ scale, float sc, const float* __restrict__ row_grad, long r,
                                                float wy, float xy, float l, float gamma) {
    return ((scale ? sc : row_grad[r]) * wy) * focal_row(xy, l, gamma).m;
}

template <bool PAD, Loss KIND, bool HAS_W>
__global__ void __launch_bounds__(256)
softmax_ce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ w, long rows,
                      int nc, int ld, long ignore, float x, float* __restrict__ lse, float* __restrict__ row_loss,
                      float* __restrict__ partial) {
    constexpr bool OPT = KIND == kOpt;
    __shared__ float sh[4];
    float loss = 0.0f, den = 0.0f;
    const long stride = (long)gridDim.x * blockDim.x;
    const int pitch = PAD ? ld : nc;
    const float W = ce_weight_sum<OPT && HAS_W>(w, nc), inv_c = 1.0f / (float)nc;        // kOpt only
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const float* __restrict__ xr = logits + r * pitch;
        float m = kNegInf, s = 0.0f, sx = 0.0f;        // running max and sum of exp(x - m); sum of w_c x_c
        for (int c = 0; c < nc; c += 4) {
            float4 v = *reinterpret_cast<const float4*>(xr + c);
            if (OPT && x > 0.0f) sx += ce_wx_chunk<HAS_W>(w, c, v, PAD ? nc - c : 4);
            if (PAD) ce_mask_tail(v, nc - c, kNegInf);
            const float vm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
            if (vm > m) { s *= __expf(m - vm); m = vm; }
            // every column so far -inf (masked classes): the exponents are taken against 0 -- exp(-inf - 0) = 0 where
            // -inf - (-inf) is NaN -- and s stays 0 until a finite column raises m.  Finite rows never come here.
            const float mz = m > kNegInf ? m : 0.0f;
            s += (__expf(v.x - mz) + __expf(v.y - mz)) + (__expf(v.z - mz) + __expf(v.w - mz));
        }
        const float l = m + __logf(s);
        lse[r] = l;
        const long y = labels[r];
        float rl = 0.0f;
        if (y != ignore && y >= 0 && y < nc) {
            const float wy = ce_w<HAS_W>(w, (int)y);   // 1 without weights: den counts the rows
            const float xy = xr[y];
            rl = KIND == kFocal ? focal_row_loss(wy, xy, l, x) : OPT ? ce_opt_row_loss(x, inv_c, wy, W, l, xy, sx) : l - xy;
            loss += rl;
            den += wy;
        }
        if (KIND != kPlain && row_loss) row_loss[r] = rl;
    }
    const float tl = block_sum(loss, sh);
    const float td = block_sum(den, sh);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = tl; partial[2 * blockIdx.x + 1] = td; }
}

template <bool PAD, Loss KIND, bool HAS_W>
__global__ void __launch_bounds__(256)
softmax_ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ lse,
                      const float* __restrict__ scale, long rows, int nc, int ld, long ignore, float* __restrict__ dlogits,
                      const float* __restrict__ w, const float* __restrict__ row_grad, float x) {
    constexpr bool OPT = KIND == kOpt;
    const float sc = (KIND == kPlain || scale) ? scale[0] : 0.0f;
    const long stride = (long)gridDim.x * blockDim.x;
    const int pitch = PAD ? ld : nc;
    const float W = ce_weight_sum<OPT && HAS_W>(w, nc), b = x * (1.0f / (float)nc);        // kOpt only
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const float* __restrict__ xr = logits + r * pitch;
        float* __restrict__ dr = dlogits + r * pitch;
        const long y = labels[r];
        const bool on = y != ignore && y >= 0 && y < nc;
        const float l = lse[r];
        float g = 0.0f;                                    // the row's upstream gradient, g w_y m for kFocal; zero for ignored rows
        if constexpr (KIND == kFocal) {
            if (on) g = focal_row_grad(scale, sc, row_grad, r, ce_w<HAS_W>(w, (int)y), xr[y], l, x);
        } else {
            g = on ? ((!OPT || scale) ? sc : row_grad[r]) : 0.0f;
        }
        const float a = (1.0f - x) * (on ? ce_w<HAS_W>(w, (int)y) : 0.0f);
        const float fp = g * (a + b * W), fa = g * a, fb = g * b;          // kOpt only
        int c = 0;
        for (; c < nc; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(xr + c);
            float4 o;
            if constexpr (OPT) {
                o = ce_opt_grad_chunk<HAS_W>(w, c, v, PAD ? nc - c : 4, l, y, fp, fa, fb);
            } else {
                o.x = (__expf(v.x - l) - (y == c ? 1.0f : 0.0f)) * g;
                o.y = (__expf(v.y - l) - (y == c + 1 ? 1.0f : 0.0f)) * g;
                o.z = (__expf(v.z - l) - (y == c + 2 ? 1.0f : 0.0f)) * g;
                o.w = (__expf(v.w - l) - (y == c + 3 ? 1.0f : 0.0f)) * g;
            }
            if (PAD) ce_mask_tail(o, nc - c, 0.0f);
            *reinterpret_cast<float4*>(dr + c) = o;
        }
        if (PAD)
            for (; c < ld; c += 4) *reinterpret_cast<float4*>(dr + c) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// Same kernels with the row (NC4 float4) held in registers: every load of a row is issued before the first use.  The
// generic kernels above walk the row with one load in flight per thread (1.2 TB/s on 8 x 480 x 640 x 40).  PAD = true:
// NC4 = ceil(nc / 4) chunks hold the valid columns.
template <int NC4, bool PAD, Loss KIND, bool HAS_W>
__global__ void __launch_bounds__(256)
softmax_ce_fwd_reg_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ w, long rows,
                          int nc_, int ld, long ignore, float x, float* __restrict__ lse, float* __restrict__ row_loss,
                          float* __restrict__ partial) {
    constexpr bool OPT = KIND == kOpt;
    __shared__ float sh[4];
    const int nc = PAD ? nc_ : NC4 * 4;
    const int pitch = PAD ? ld : NC4 * 4;
    float loss = 0.0f, den = 0.0f;
    const long stride = (long)gridDim.x * blockDim.x;
    const float W = ce_weight_sum<OPT && HAS_W>(w, nc), inv_c = 1.0f / (float)nc;        // kOpt only
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const float4* __restrict__ xr = reinterpret_cast<const float4*>(logits + r * pitch);
        float4 v[NC4];
#pragma unroll
        for (int c = 0; c < NC4; ++c) v[c] = xr[c];
        const long y = labels[r];
        float sx = 0.0f;
        if (OPT && x > 0.0f) {
#pragma unroll
            for (int c = 0; c < NC4; ++c) sx += ce_wx_chunk<HAS_W>(w, 4 * c, v[c], (PAD && c == NC4 - 1) ? nc - 4 * c : 4);
        }
        if (PAD) ce_mask_tail(v[NC4 - 1], nc - 4 * (NC4 - 1), kNegInf);
        float m = kNegInf;
#pragma unroll
        for (int c = 0; c < NC4; ++c) m = fmaxf(m, fmaxf(fmaxf(v[c].x, v[c].y), fmaxf(v[c].z, v[c].w)));
        float s = 0.0f, xy = 0.0f;
#pragma unroll
        for (int c = 0; c < NC4; ++c) {
            s += (__expf(v[c].x - m) + __expf(v[c].y - m)) + (__expf(v[c].z - m) + __expf(v[c].w - m));
            if (KIND != kFocal) xy = SIGMA_CE_PICK(v[c], 4 * c, y, xy);      // kFocal picks under the label test: fewer registers
        }
        const float l = m + __logf(s);
        lse[r] = l;
        float rl = 0.0f;
        if (y != ignore && y >= 0 && y < nc) {
            const float wy = ce_w<HAS_W>(w, (int)y);   // 1 without weights: den counts the rows
            rl = KIND == kFocal ? focal_row_loss(wy, ce_pick<NC4>(v, y), l, x) : OPT ? ce_opt_row_loss(x, inv_c, wy, W, l, xy, sx) : l - xy;
            loss += rl;
            den += wy;
        }
        if (KIND != kPlain && row_loss) row_loss[r] = rl;
    }
    const float tl = block_sum(loss, sh);
    const float td = block_sum(den, sh);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = tl; partial[2 * blockIdx.x + 1] = td; }
}

template <int NC4, bool PAD, Loss KIND, bool HAS_W>
__global__ void __launch_bounds__(256)
softmax_ce_bwd_reg_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ lse,
                          const float* __restrict__ scale, long rows, int nc_, int ld, long ignore, float* __restrict__ dlogits,
                          const float* __restrict__ w, const float* __restrict__ row_grad, float x) {
    constexpr bool OPT = KIND == kOpt;
    const int nc = PAD ? nc_ : NC4 * 4;
    const int pitch = PAD ? ld : NC4 * 4;
    const float sc = (KIND == kPlain || scale) ? scale[0] : 0.0f;
    const long stride = (long)gridDim.x * blockDim.x;
    const float W = ce_weight_sum<OPT && HAS_W>(w, nc), b = x * (1.0f / (float)nc);        // kOpt only
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const float4* __restrict__ xr = reinterpret_cast<const float4*>(logits + r * pitch);
        float4* __restrict__ dr = reinterpret_cast<float4*>(dlogits + r * pitch);
        float4 v[NC4];
#pragma unroll
        for (int c = 0; c < NC4; ++c) v[c] = xr[c];
        const long y = labels[r];
        const float l = lse[r];
        const bool on = y != ignore && y >= 0 && y < nc;
        float g = 0.0f;                                    // the row's upstream gradient, g w_y m for kFocal; zero for ignored rows
        if constexpr (KIND == kFocal) {
            if (on) g = focal_row_grad(scale, sc, row_grad, r, ce_w<HAS_W>(w, (int)y), ce_pick<NC4>(v, y), l, x);
        } else {
            g = on ? ((!OPT || scale) ? sc : row_grad[r]) : 0.0f;
        }
        const float a = (1.0f - x) * (on ? ce_w<HAS_W>(w, (int)y) : 0.0f);
        const float fp = g * (a + b * W), fa = g * a, fb = g * b;          // kOpt only
#pragma unroll
        for (int c = 0; c < NC4; ++c) {
            const bool tail = PAD && c == NC4 - 1;
            float4 o;
            if constexpr (OPT) {
                o = ce_opt_grad_chunk<HAS_W>(w, 4 * c, v[c], tail ? nc - 4 * c : 4, l, y, fp, fa, fb);
            } else {
                o.x = (__expf(v[c].x - l) - (y == 4 * c ? 1.0f : 0.0f)) * g;
                o.y = (__expf(v[c].y - l) - (y == 4 * c + 1 ? 1.0f : 0.0f)) * g;
                o.z = (__expf(v[c].z - l) - (y == 4 * c + 2 ? 1.0f : 0.0f)) * g;
                o.w = (__expf(v[c].w - l) - (y == 4 * c + 3 ? 1.0f : 0.0f)) * g;
            }
            if (tail) ce_mask_tail(o, nc - 4 * c, 0.0f);
            dr[c] = o;
        }
        if (PAD)
            for (int c = NC4; c < (ld >> 2); ++c) dr[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

#undef SIGMA_CE_PICK

// NC4 = ceil(classes / 4) chunks held in registers up to 64 classes
template <typename F>
bool dispatch_nc4(int nc4, F&& f) {
    switch (nc4) {
#define SIGMA_NC4(N) case N: f(std::integral_constant<int, N>()); return true;
        SIGMA_NC4(1) SIGMA_NC4(2) SIGMA_NC4(3) SIGMA_NC4(4) SIGMA_NC4(5) SIGMA_NC4(6) SIGMA_NC4(7) SIGMA_NC4(8)
        SIGMA_NC4(9) SIGMA_NC4(10) SIGMA_NC4(11) SIGMA_NC4(12) SIGMA_NC4(13) SIGMA_NC4(14) SIGMA_NC4(15) SIGMA_NC4(16)
#undef SIGMA_NC4
        default: return false;
    }
}

// the two flags of a loss launch as types
template <typename F>
void dispatch_flags(bool pad, bool has_w, F&& f) {
    if (pad && has_w) f(std::true_type(), std::true_type());
    else if (pad) f(std::true_type(), std::false_type());
    else if (has_w) f(std::false_type(), std::true_type());
    else f(std::false_type(), std::false_type());
}

// ---- backward of  y = a + x * s  with a per-channel s on channels-last rows (CVSSDecoderBlock, vmamba.py:1800-1805) ------
// dx = dy * s and ds += sum over rows of dy * x, one pass over dy and x.  A thread keeps ONE 16-byte column chunk for the
// whole kernel (chunk = tid % (C / 4), row slot = tid / (C / 4); 256 / (C / 4) rows per block iteration), so its part of
// ds lives in four registers; the row slots of a block meet in LDS and one thread per chunk adds the block's sum to ds
// (float atomics: grid x C / 4 of them).  C % 4 == 0, C <= 1024.
// DET (sigma_colscale_bwd_ws): the block's sum is stored to row blockIdx.x of `ds` = the workspace instead.
template <bool DET>
__device__ __forceinline__ void colscale_bwd_body(const float* __restrict__ dy, const float* __restrict__ x,
                                                  const float* __restrict__ s, float* __restrict__ dx,
                                                  float* __restrict__ ds, long rows, int C) {
    extern __shared__ float part[];                       // [slots][C]
    const int chunks = C >> 2;
    const int slots = 256 / chunks;
    const int slot = threadIdx.x / chunks, ch = threadIdx.x - slot * chunks;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (slot < slots) {
        const float4 sv = *reinterpret_cast<const float4*>(s + 4 * ch);
        for (long r = (long)blockIdx.x * slots + slot; r < rows; r += (long)gridDim.x * slots) {
            const float4 g = *reinterpret_cast<const float4*>(dy + r * C + 4 * ch);
            const float4 xv = *reinterpret_cast<const float4*>(x + r * C + 4 * ch);
            *reinterpret_cast<float4*>(dx + r * C + 4 * ch) = make_float4(g.x * sv.x, g.y * sv.y, g.z * sv.z, g.w * sv.w);
            acc.x = fmaf(g.x, xv.x, acc.x); acc.y = fmaf(g.y, xv.y, acc.y); acc.z = fmaf(g.z, xv.z, acc.z); acc.w = fmaf(g.w, xv.w, acc.w);
        }
        *reinterpret_cast<float4*>(part + slot * C + 4 * ch) = acc;
    }
    __syncthreads();
    if (slot == 0) {
        float4 t = acc;
        for (int k = 1; k < slots; ++k) {
            const float4 o = *reinterpret_cast<const float4*>(part + k * C + 4 * ch);
            t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
        }
        if constexpr (DET) *reinterpret_cast<float4*>(ds + (long)blockIdx.x * C + 4 * ch) = t;
        else { atomicAdd(ds + 4 * ch, t.x); atomicAdd(ds + 4 * ch + 1, t.y); atomicAdd(ds + 4 * ch + 2, t.z); atomicAdd(ds + 4 * ch + 3, t.w); }
    }
}

__global__ void __launch_bounds__(256) colscale_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ s, float* __restrict__ dx,
                                                           float* __restrict__ ds, long rows, int C) {
    colscale_bwd_body<false>(dy, x, s, dx, ds, rows, C);
}

__global__ void __launch_bounds__(256) colscale_bwd_part_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                const float* __restrict__ s, float* __restrict__ dx,
                                                                float* __restrict__ ws, long rows, int C) {
    colscale_bwd_body<true>(dy, x, s, dx, ws, rows, C);
}

// ds[c] = sum over the `blocks` rows of ws in a fixed order: thread (x, y) of a 64 x 16 block adds the rows y, y + 16, ...
// of column blockIdx.x * 64 + x, then the 16 partial sums meet in LDS and are added y = 0 .. 15
__global__ void __launch_bounds__(1024) colscale_reduce_kernel(const float* __restrict__ ws, float* __restrict__ ds, int blocks, int C) {
    __shared__ float part[16][64];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + x;
    float acc = 0.0f;
    if (c < C)
        for (int b = y; b < blocks; b += 16) acc += ws[(long)b * C + c];
    part[y][x] = acc;
    __syncthreads();
    if (y == 0 && c < C) {
        float t = part[0][x];
        for (int k = 1; k < 16; ++k) t += part[k][x];
        ds[c] = t;
    }
}

// blocks of the colscale backward (two workgroups per CU: every block ends with C atomics on the same C addresses)
long colscale_grid(long rows, int channels) {
    const int slots = 256 / (channels / 4);
    long grid = (rows + slots - 1) / slots;
    return grid > 512 ? 512 : grid;
}

unsigned stream_grid(long work_items) {
    long b = (work_items + 255) / 256;
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// the arguments of the plain loss as the launchers take them: no option set (the backward only reads lse)
sigma_ce_opt_params ce_plain(const float* logits, const int64_t* labels, int64_t rows, int32_t classes, int32_t ld, int64_t ignore_index,
                             const float* lse, float* partial, const float* scale, float* dlogits) {
    sigma_ce_opt_params p = {};
    p.rows = rows; p.classes = classes; p.ld = ld; p.ignore_index = ignore_index;
    p.logits = logits; p.labels = labels; p.lse = const_cast<float*>(lse);
    p.partial = partial; p.scale = scale; p.dlogits = dlogits;
    return p;
}

// One launcher per direction for the three kinds; `x` is the kernels' float (0 for kPlain, whose `p` holds weight, row_loss
// and row_grad NULL).  The arguments are checked by the entry points.  Rows of up to 64 classes go to the register kernels.
template <Loss KIND>
int ce_launch_fwd(const sigma_ce_opt_params& p, float x, void* stream) {
    // every one of the SIGMA_CE_BLOCKS workgroups writes its (loss, weight or count) pair, rows or not: the caller adds them up
    const dim3 grid(SIGMA_CE_BLOCKS), block(256);
    dispatch_flags(p.ld != p.classes, KIND != kPlain && p.weight != nullptr, [&](auto pad, auto has_w) {
        constexpr bool PAD = decltype(pad)::value, HAS_W = KIND != kPlain && decltype(has_w)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, static_cast<hipStream_t>(stream), p.logits, p.labels, p.weight, (long)p.rows,
                               (int)p.classes, (int)p.ld, (long)p.ignore_index, x, p.lse, p.row_loss, p.partial);
        };
        if (!dispatch_nc4((p.classes + 3) / 4, [&](auto n) { launch(softmax_ce_fwd_reg_kernel<decltype(n)::value, PAD, KIND, HAS_W>); }))
            launch(softmax_ce_fwd_kernel<PAD, KIND, HAS_W>);
    });
    return launched("softmax_ce_fwd_kernel");
}

template <Loss KIND>
int ce_launch_bwd(const sigma_ce_opt_params& p, float x, void* stream) {
    const dim3 grid(stream_grid(p.rows)), block(256);
    dispatch_flags(p.ld != p.classes, KIND != kPlain && p.weight != nullptr, [&](auto pad, auto has_w) {
        constexpr bool PAD = decltype(pad)::value, HAS_W = KIND != kPlain && decltype(has_w)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, static_cast<hipStream_t>(stream), p.logits, p.labels, p.lse, p.scale, (long)p.rows,
                               (int)p.classes, (int)p.ld, (long)p.ignore_index, p.dlogits, p.weight, p.row_grad, x);
        };
        if (!dispatch_nc4((p.classes + 3) / 4, [&](auto n) { launch(softmax_ce_bwd_reg_kernel<decltype(n)::value, PAD, KIND, HAS_W>); }))
            launch(softmax_ce_bwd_kernel<PAD, KIND, HAS_W>);
    });
    return launched("softmax_ce_bwd_kernel");
}

}  // namespace
}  // namespace sigma

extern "C" {

int sigma_plane_pool(const float* x, int64_t planes, int64_t hw, float* mean, float* max, float* count, void* stream) {
    if (planes < 0 || hw <= 0 || planes > 2147483647L)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "planes %lld must be in [0, 2^31 - 1] and hw %lld positive", (long long)planes, (long long)hw);
    if (planes == 0) return SIGMA_OPS_OK;
    if (!x || !mean || !max || !count) return sigma::fail(SIGMA_OPS_ERR_ARG, "x, mean, max and count must be non-NULL device pointers");
    const int vec = (hw % 4 == 0 && sigma::aligned(x, 16)) ? 1 : 0;
    hipLaunchKernelGGL(sigma::plane_pool_kernel, dim3((unsigned)planes), dim3(256), 0, static_cast<hipStream_t>(stream), x, (long)hw, vec,
                       mean, max, count);
    return sigma::launched("plane_pool_kernel");
}

int sigma_plane_dot(const float* a, const float* b, float* out, int64_t planes, int64_t hw, void* stream) {
    if (planes < 0 || hw <= 0 || planes > 2147483647L)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "planes %lld must be in [0, 2^31 - 1] and hw %lld positive", (long long)planes, (long long)hw);
    if (planes == 0) return SIGMA_OPS_OK;
    if (!a || !b || !out) return sigma::fail(SIGMA_OPS_ERR_ARG, "a, b and out must be non-NULL device pointers");
    const int vec = (hw % 4 == 0 && sigma::aligned(a, 16) && sigma::aligned(b, 16)) ? 1 : 0;
    hipLaunchKernelGGL(sigma::plane_dot_kernel, dim3((unsigned)planes), dim3(256), 0, static_cast<hipStream_t>(stream), a, b, (long)hw, vec, out);
    return sigma::launched("plane_dot_kernel");
}

int sigma_plane_scale(const float* x, const float* scale, float* out, int64_t planes, int64_t hw, void* stream) {
    if (planes < 0 || hw <= 0) return sigma::fail(SIGMA_OPS_ERR_ARG, "planes %lld must not be negative and hw %lld be positive", (long long)planes, (long long)hw);
    if (planes == 0) return SIGMA_OPS_OK;
    if (!x || !scale || !out) return sigma::fail(SIGMA_OPS_ERR_ARG, "x, scale and out must be non-NULL device pointers");
    const int vec = (hw % 4 == 0 && sigma::aligned(x, 16) && sigma::aligned(out, 16)) ? 1 : 0;
    const long work = vec ? planes * (hw / 4) : planes * hw;
    hipLaunchKernelGGL(sigma::plane_scale_kernel, dim3(sigma::stream_grid(work)), dim3(256), 0, static_cast<hipStream_t>(stream), x, scale, out,
                       (long)planes, (long)hw, vec);
    return sigma::launched("plane_scale_kernel");
}

int sigma_colscale_bwd(const float* dy, const float* x, const float* scale, float* dx, float* dscale, int64_t rows, int32_t channels,
                       void* stream) {
    if (rows < 0 || channels <= 0 || channels % 4 != 0 || channels > 1024)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "rows %lld must not be negative and channels %d be a multiple of 4 in (0, 1024]", (long long)rows, channels);
    if (rows == 0) return SIGMA_OPS_OK;
    if (!dy || !x || !scale || !dx || !dscale) return sigma::fail(SIGMA_OPS_ERR_ARG, "dy, x, scale, dx and dscale must be non-NULL device pointers");
    if (!sigma::aligned(dy, 16) || !sigma::aligned(x, 16) || !sigma::aligned(scale, 16) || !sigma::aligned(dx, 16))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "dy, x, scale and dx must be 16-byte aligned");
    const int slots = 256 / (channels / 4);
    const long grid = sigma::colscale_grid((long)rows, channels);
    hipLaunchKernelGGL(sigma::colscale_bwd_kernel, dim3((unsigned)grid), dim3(256), (size_t)slots * channels * sizeof(float),
                       static_cast<hipStream_t>(stream), dy, x, scale, dx, dscale, (long)rows, (int)channels);
    return sigma::launched("colscale_bwd_kernel");
}

int64_t sigma_colscale_bwd_workspace_bytes(int64_t rows, int32_t channels) {
    if (rows < 0 || channels <= 0 || channels % 4 != 0 || channels > 1024)
        return sigma::fail(-1, "rows %lld must not be negative and channels %d be a multiple of 4 in (0, 1024]", (long long)rows, channels);
    return (int64_t)sigma::colscale_grid((long)rows, channels) * channels * (int64_t)sizeof(float);
}

int sigma_colscale_bwd_ws(const float* dy, const float* x, const float* scale, float* dx, float* dscale, int64_t rows, int32_t channels,
                          void* workspace, int64_t workspace_bytes, void* stream) {
    if (rows < 0 || channels <= 0 || channels % 4 != 0 || channels > 1024)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "rows %lld must not be negative and channels %d be a multiple of 4 in (0, 1024]", (long long)rows, channels);
    if (!dscale) return sigma::fail(SIGMA_OPS_ERR_ARG, "dscale is NULL");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (rows == 0) return sigma::launched("hipMemsetAsync of dscale", hipMemsetAsync(dscale, 0, (size_t)channels * sizeof(float), st));
    if (!dy || !x || !scale || !dx) return sigma::fail(SIGMA_OPS_ERR_ARG, "dy, x, scale and dx must be non-NULL device pointers");
    if (!sigma::aligned(dy, 16) || !sigma::aligned(x, 16) || !sigma::aligned(scale, 16) || !sigma::aligned(dx, 16))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "dy, x, scale and dx must be 16-byte aligned");
    if (!workspace || !sigma::aligned(workspace, 16) || workspace_bytes < sigma_colscale_bwd_workspace_bytes(rows, channels))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "a 16-byte aligned workspace of %lld bytes is required (got %p, %lld bytes)",
                           (long long)sigma_colscale_bwd_workspace_bytes(rows, channels), workspace, (long long)workspace_bytes);
    const int slots = 256 / (channels / 4);
    const long grid = sigma::colscale_grid((long)rows, channels);
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(sigma::colscale_bwd_part_kernel, dim3((unsigned)grid), dim3(256), (size_t)slots * channels * sizeof(float),
                       st, dy, x, scale, dx, ws, (long)rows, (int)channels);
    if (const int rc = sigma::launched("colscale_bwd_part_kernel")) return rc;
    hipLaunchKernelGGL(sigma::colscale_reduce_kernel, dim3((unsigned)((channels + 63) / 64)), dim3(1024), 0, st, ws, dscale,
                       (int)grid, (int)channels);
    return sigma::launched("colscale_reduce_kernel");
}

int sigma_plane_gate_bwd(const sigma_gate_bwd_params* p, void* stream) {
    if (!p) return sigma::fail(SIGMA_OPS_ERR_ARG, "params is NULL");
    if (p->planes < 0 || p->hw <= 0)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "planes %lld must not be negative and hw %lld be positive", (long long)p->planes, (long long)p->hw);
    if (p->planes == 0) return SIGMA_OPS_OK;
    if (!p->g || !p->x || !p->scale || !p->dmean || !p->dmax || !p->max || !p->count || !p->dx)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "g, x, scale, dmean, dmax, max, count and dx must be non-NULL device pointers");
    sigma::GateBwdArgs a{p->g, p->x, p->scale, p->dmean, p->dmax, p->max, p->count, p->dx, (long)p->planes, (long)p->hw, 0};
    a.vec = (p->hw % 4 == 0 && sigma::aligned(p->g, 16) && sigma::aligned(p->x, 16) && sigma::aligned(p->dx, 16)) ? 1 : 0;
    const long work = a.vec ? a.planes * (a.hw / 4) : a.planes * a.hw;
    hipLaunchKernelGGL(sigma::plane_gate_bwd_kernel, dim3(sigma::stream_grid(work)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return sigma::launched("plane_gate_bwd_kernel");
}

int sigma_softmax_ce_fwd(const float* logits, const int64_t* labels, int64_t rows, int32_t classes, int64_t ignore_index, float* lse,
                         float* partial, void* stream) {
    if (classes <= 0 || classes % 4 != 0) return sigma::fail(SIGMA_OPS_ERR_ARG, "classes %d must be a positive multiple of 4 (other counts: the _ld entry points)", classes);
    return sigma_softmax_ce_fwd_ld(logits, labels, rows, classes, classes, ignore_index, lse, partial, stream);
}

int sigma_softmax_ce_bwd(const float* logits, const int64_t* labels, const float* lse, const float* scale, int64_t rows, int32_t classes,
                         int64_t ignore_index, float* dlogits, void* stream) {
    if (classes <= 0 || classes % 4 != 0) return sigma::fail(SIGMA_OPS_ERR_ARG, "classes %d must be a positive multiple of 4 (other counts: the _ld entry points)", classes);
    return sigma_softmax_ce_bwd_ld(logits, labels, lse, scale, rows, classes, classes, ignore_index, dlogits, stream);
}

// ld == classes: the PAD = false kernels, i.e. what sigma_softmax_ce_fwd / _bwd have always launched
int sigma_softmax_ce_fwd_ld(const float* logits, const int64_t* labels, int64_t rows, int32_t classes, int32_t ld, int64_t ignore_index,
                            float* lse, float* partial, void* stream) {
    if (rows < 0 || classes < 1 || ld % 4 != 0 || ld < classes)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "rows %lld must not be negative, classes %d be at least 1 and ld %d a multiple of 4, at least classes",
                           (long long)rows, classes, ld);
    if (!partial) return sigma::fail(SIGMA_OPS_ERR_ARG, "partial is NULL");
    if (rows > 0 && (!logits || !labels || !lse || !sigma::aligned(logits, 16)))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "logits, labels and lse must be non-NULL device pointers, logits 16-byte aligned");
    const sigma_ce_opt_params p = sigma::ce_plain(logits, labels, rows, classes, ld, ignore_index, lse, partial, nullptr, nullptr);
    return sigma::ce_launch_fwd<sigma::kPlain>(p, 0.0f, stream);
}

int sigma_softmax_ce_bwd_ld(const float* logits, const int64_t* labels, const float* lse, const float* scale, int64_t rows, int32_t classes,
                            int32_t ld, int64_t ignore_index, float* dlogits, void* stream) {
    if (rows < 0 || classes < 1 || ld % 4 != 0 || ld < classes)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "rows %lld must not be negative, classes %d be at least 1 and ld %d a multiple of 4, at least classes",
                           (long long)rows, classes, ld);
    if (rows == 0) return SIGMA_OPS_OK;
    if (!logits || !labels || !lse || !scale || !dlogits || !sigma::aligned(logits, 16) || !sigma::aligned(dlogits, 16))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "logits, labels, lse, scale and dlogits must be non-NULL device pointers, logits and dlogits 16-byte aligned");
    const sigma_ce_opt_params p = sigma::ce_plain(logits, labels, rows, classes, ld, ignore_index, lse, nullptr, scale, dlogits);
    return sigma::ce_launch_bwd<sigma::kPlain>(p, 0.0f, stream);
}

// everything the _opt_ and _focal_ entry points check alike in both directions, before any launch.  gamma (focal only, else
// NULL): smoothing is refused, and an exponent that is NaN, negative or in (0, 1)
static int ce_opt_check(const sigma_ce_opt_params* p, const float* gamma) {
    if (!p) return sigma::fail(SIGMA_OPS_ERR_ARG, "params is NULL");
    if (p->rows < 0 || p->classes < 1 || p->ld % 4 != 0 || p->ld < p->classes)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "rows %lld must not be negative, classes %d be at least 1 and ld %d a multiple of 4, at least classes",
                           (long long)p->rows, p->classes, p->ld);
    if (!(p->label_smoothing >= 0.0f && p->label_smoothing <= 1.0f))      // NaN fails both
        return sigma::fail(SIGMA_OPS_ERR_ARG, "label_smoothing %g must be in [0, 1]", (double)p->label_smoothing);
    if (!sigma::aligned(p->weight, 4) || !sigma::aligned(p->lse, 4) || !sigma::aligned(p->row_loss, 4) || !sigma::aligned(p->partial, 4) ||
        !sigma::aligned(p->scale, 4) || !sigma::aligned(p->row_grad, 4) || !sigma::aligned(p->labels, 8))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "alignment: weight, lse, row_loss, partial, scale and row_grad need 4 bytes, labels 8");
    if (gamma) {
        if (p->label_smoothing != 0.0f) return sigma::fail(SIGMA_OPS_ERR_ARG, "the focal loss takes no label_smoothing (got %g)", (double)p->label_smoothing);
        if (!(*gamma == 0.0f || (*gamma >= 1.0f && *gamma <= 3.0e38f)))      // NaN and inf fail both
            return sigma::fail(SIGMA_OPS_ERR_ARG, "gamma %g must be 0 or finite and at least 1", (double)*gamma);
    }
    return SIGMA_OPS_OK;
}

static int ce_opt_fwd_check(const sigma_ce_opt_params* p, const float* gamma) {
    if (const int rc = ce_opt_check(p, gamma)) return rc;
    if (!p->partial) return sigma::fail(SIGMA_OPS_ERR_ARG, "partial is NULL");
    if (p->rows > 0 && (!p->logits || !p->labels || !p->lse || !sigma::aligned(p->logits, 16)))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "logits, labels and lse must be non-NULL device pointers, logits 16-byte aligned");
    return SIGMA_OPS_OK;
}

// no rows: nothing is launched and no buffer is looked at
static int ce_opt_bwd_check(const sigma_ce_opt_params* p, const float* gamma) {
    if (const int rc = ce_opt_check(p, gamma)) return rc;
    if ((p->scale != nullptr) == (p->row_grad != nullptr))      // one of them, not both
        return sigma::fail(SIGMA_OPS_ERR_ARG, "exactly one of scale (%p) and row_grad (%p) must be given", (const void*)p->scale, (const void*)p->row_grad);
    if (p->rows > 0 && (!p->logits || !p->labels || !p->lse || !p->dlogits || !sigma::aligned(p->logits, 16) || !sigma::aligned(p->dlogits, 16)))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "logits, labels, lse and dlogits must be non-NULL device pointers, logits and dlogits 16-byte aligned");
    return SIGMA_OPS_OK;
}

int sigma_softmax_ce_opt_fwd(const sigma_ce_opt_params* p, void* stream) {
    if (const int rc = ce_opt_fwd_check(p, nullptr)) return rc;
    return sigma::ce_launch_fwd<sigma::kOpt>(*p, p->label_smoothing, stream);
}

int sigma_softmax_ce_opt_bwd(const sigma_ce_opt_params* p, void* stream) {
    if (const int rc = ce_opt_bwd_check(p, nullptr)) return rc;
    return p->rows == 0 ? SIGMA_OPS_OK : sigma::ce_launch_bwd<sigma::kOpt>(*p, p->label_smoothing, stream);
}

int sigma_softmax_focal_fwd(const sigma_ce_opt_params* p, float gamma, void* stream) {
    if (const int rc = ce_opt_fwd_check(p, &gamma)) return rc;
    return sigma::ce_launch_fwd<sigma::kFocal>(*p, gamma, stream);
}

int sigma_softmax_focal_bwd(const sigma_ce_opt_params* p, float gamma, void* stream) {
    if (const int rc = ce_opt_bwd_check(p, &gamma)) return rc;
    return p->rows == 0 ? SIGMA_OPS_OK : sigma::ce_launch_bwd<sigma::kFocal>(*p, gamma, stream);
}

}  // extern "C"
