// segmetric.hip -- the evaluator's per-image bookkeeping on the device: multi-scale score sum, arg-max, confusion matrix.
//
// Reference: Evaluator.sliding_eval_rgbX (engine/evaluator.py:433-450) adds the (H, W, C) float32 scores of every scale
// into np.zeros((H, W, C)) -- float64 -- and takes argmax(2); SegEvaluator.func_per_iteration (eval.py:22-30) then calls
// hist_info (utils/metric.py:8-15): k = (gt >= 0) & (gt < n_cl), labeled = sum(k), correct = sum(pred[k] == gt[k]),
// hist = bincount(n_cl * gt[k] + pred[k]).  Here (include/sigma_ops.h):
//
//   seg_accumulate        acc[c, p] (+)= (double)score[c, p], one launch per scale; the first scale writes 0.0 + score
//                         (numpy's zeros + score, bit for bit, -0.0 included), so no zero fill is needed
//   seg_confusion         ONE pass over the pixels: a lane per pixel (two when the planes allow 16-byte loads) walks
//                         the C class planes -- every load instruction of a wave reads 512 (1024) contiguous bytes --
//                         keeps the first maximum (strict >) and the first NaN, writes pred, reads gt and counts
//
// Layout: class-planar (C, pixels), which is what the evaluator's device score is before its permute to (H, W, C).
// With C = 9..40 a cross-lane reduction per pixel would spend 4-6 shuffle levels on fewer lanes than a wave; a lane
// per pixel needs none and the compare chain is C - 1 v_cmp_gt_f64 + v_cmp_u_f64 per pixel (fp64 compares are full
// rate on CDNA), far below the float64 stream: 8 * C bytes per pixel, 98 MB for a 480 x 640 x 40 image.
//
// Counts: per-workgroup uint32 histograms in LDS (ds_add_u32; SIGMA_SEG_LDS_HIST_BYTES = 32 KiB, n_cl <= 90), then
// every non-zero bin is added to the int64 global histogram (global 64-bit integer atomics).  Above the LDS budget the
// pixels go straight to the global histogram.  Integer adds are exact and associative: the result does not depend on
// the order the workgroups arrive in, so deterministic mode needs nothing extra.  Overflow: a workgroup visits fewer
// than 2^31 pixels (pixels < 2^31 is checked), so no uint32 LDS bin or count can wrap; the int64 outputs wrap after
// 2^63 pixels summed over all the calls a caller accumulates into them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ops_host.h"

namespace sigma {
namespace {

constexpr int kSegThreads = 256;
constexpr unsigned kSegMaxGrid = 512;       // two workgroups per CU; a lane then walks ~1-3 pixels of a 480 x 640 image

template <int V>
__global__ __launch_bounds__(kSegThreads) void seg_accumulate_kernel(const float* __restrict__ score, double* __restrict__ acc,
                                                                     long pixels, long s_stride, long a_stride, int first) {
    const float* s = score + (long)blockIdx.y * s_stride;
    double* a = acc + (long)blockIdx.y * a_stride;
    const long n = pixels / V;
    const long step = (long)gridDim.x * kSegThreads;
    for (long i = (long)blockIdx.x * kSegThreads + threadIdx.x; i < n; i += step) {
        if constexpr (V == 4) {
            const float4 v = reinterpret_cast<const float4*>(s)[i];
            double2* d = reinterpret_cast<double2*>(a + 4 * i);
            double2 lo = first ? make_double2(0.0, 0.0) : d[0];
            double2 hi = first ? make_double2(0.0, 0.0) : d[1];
            lo.x += (double)v.x;
            lo.y += (double)v.y;
            hi.x += (double)v.z;
            hi.y += (double)v.w;
            d[0] = lo;
            d[1] = hi;
        } else {
            const double prev = first ? 0.0 : a[i];      // 0.0 + x is not x for x = -0.0: kept, as numpy computes it
            a[i] = prev + (double)s[i];
        }
    }
}

struct ConfArgs {
    const double* acc;
    long stride;            // elements between class planes of acc
    void* pred;
    const void* gt;
    unsigned long long* hist;
    unsigned long long* counts;
    long pixels;
    int classes;
    int n_cl;
};

// numpy's argmax over the C planes for PIX adjacent pixels starting at p: the first maximum (strict >), or the first NaN
template <int PIX>
__device__ __forceinline__ void argmax_planes(const ConfArgs& a, long p, int* idx) {
    double best[PIX];
    bool nan[PIX];
    const double* base = a.acc + p;
    if constexpr (PIX == 2) {
        const double2 v = *reinterpret_cast<const double2*>(base);
        best[0] = v.x;
        best[1] = v.y;
    } else {
        best[0] = base[0];
    }
#pragma unroll
    for (int k = 0; k < PIX; ++k) {
        idx[k] = 0;
        nan[k] = isnan(best[k]);
    }
    constexpr int U = 8;                             // eight plane loads in flight before the compare chain
    for (int c0 = 1; c0 < a.classes; c0 += U) {
        double v[U][PIX];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c0 + u < a.classes) {
                const double* q = base + (long)(c0 + u) * a.stride;
                if constexpr (PIX == 2) {
                    const double2 w = *reinterpret_cast<const double2*>(q);
                    v[u][0] = w.x;
                    v[u][1] = w.y;
                } else {
                    v[u][0] = q[0];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c0 + u < a.classes) {
#pragma unroll
                for (int k = 0; k < PIX; ++k) {
                    const bool vn = isnan(v[u][k]);
                    if (!nan[k] && (vn || v[u][k] > best[k])) {
                        best[k] = v[u][k];
                        idx[k] = c0 + u;
                        nan[k] = vn;
                    }
                }
            }
        }
    }
}

// FROM_ACC: pred = argmax of acc (written when a.pred != NULL); else pred is read from a.pred.  LDS_HIST: per-workgroup
// uint32 bins in LDS; else int64 atomics into the global histogram.
template <typename GT, typename PR, bool FROM_ACC, bool LDS_HIST, int PIX>
__global__ __launch_bounds__(kSegThreads) void seg_confusion_kernel(ConfArgs a) {
    extern __shared__ unsigned int bins[];
    __shared__ unsigned int wg_counts[3];
    const int nb = a.n_cl * a.n_cl;
    if constexpr (LDS_HIST) {
        for (int i = threadIdx.x; i < nb; i += kSegThreads) bins[i] = 0u;
    }
    if (threadIdx.x < 3) wg_counts[threadIdx.x] = 0u;
    __syncthreads();

    unsigned int labeled = 0, correct = 0, invalid = 0;
    const long groups = a.pixels / PIX;
    const long step = (long)gridDim.x * kSegThreads;
    for (long g = (long)blockIdx.x * kSegThreads + threadIdx.x; g < groups; g += step) {
        const long p = g * PIX;
        long pr[PIX];
        if constexpr (FROM_ACC) {
            int idx[PIX];
            argmax_planes<PIX>(a, p, idx);
#pragma unroll
            for (int k = 0; k < PIX; ++k) {
                pr[k] = idx[k];
                if (a.pred) static_cast<PR*>(a.pred)[p + k] = (PR)idx[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < PIX; ++k) pr[k] = (long)static_cast<const PR*>(a.pred)[p + k];
        }
        if (!a.gt) continue;                              // arg-max only (uniform over the launch)
#pragma unroll
        for (int k = 0; k < PIX; ++k) {
            const long t = (long)static_cast<const GT*>(a.gt)[p + k];
            if (t >= 0 && t < a.n_cl) {
                ++labeled;
                correct += pr[k] == t ? 1u : 0u;
                if (pr[k] >= 0 && pr[k] < a.n_cl) {
                    const int bin = (int)t * a.n_cl + (int)pr[k];
                    if constexpr (LDS_HIST) atomicAdd(&bins[bin], 1u);
                    else atomicAdd(&a.hist[bin], 1ull);
                } else {
                    ++invalid;
                }
            }
        }
    }
    if (labeled) atomicAdd(&wg_counts[0], labeled);
    if (correct) atomicAdd(&wg_counts[1], correct);
    if (invalid) atomicAdd(&wg_counts[2], invalid);
    __syncthreads();
    if (LDS_HIST && a.gt) {
        for (int i = threadIdx.x; i < nb; i += kSegThreads) {
            const unsigned int b = bins[i];
            if (b) atomicAdd(&a.hist[i], (unsigned long long)b);
        }
    }
    if (a.gt && threadIdx.x < 3) {
        const unsigned int c = wg_counts[threadIdx.x];
        if (c) atomicAdd(&a.counts[threadIdx.x], (unsigned long long)c);
    }
}

template <typename GT, typename PR, bool FROM_ACC, bool LDS_HIST>
void launch_confusion(const ConfArgs& a, int pix, hipStream_t s) {
    const long groups = a.pixels / pix;
    long grid = (groups + kSegThreads - 1) / kSegThreads;
    if (grid > (long)kSegMaxGrid) grid = kSegMaxGrid;
    if (grid < 1) grid = 1;
    const size_t lds = LDS_HIST ? (size_t)a.n_cl * a.n_cl * sizeof(unsigned int) : 0;
    if (pix == 2)
        hipLaunchKernelGGL((seg_confusion_kernel<GT, PR, FROM_ACC, LDS_HIST, 2>), dim3((unsigned)grid), dim3(kSegThreads), lds, s, a);
    else
        hipLaunchKernelGGL((seg_confusion_kernel<GT, PR, FROM_ACC, LDS_HIST, 1>), dim3((unsigned)grid), dim3(kSegThreads), lds, s, a);
}

template <typename GT, typename PR>
void dispatch_confusion(const ConfArgs& a, bool from_acc, bool lds_hist, int pix, hipStream_t s) {
    if (from_acc) {
        if (lds_hist) launch_confusion<GT, PR, true, true>(a, pix, s);
        else launch_confusion<GT, PR, true, false>(a, pix, s);
    } else {
        if (lds_hist) launch_confusion<GT, PR, false, true>(a, 1, s);
        else launch_confusion<GT, PR, false, false>(a, 1, s);
    }
}

}  // namespace
}  // namespace sigma

extern "C" {

int sigma_seg_accumulate(const sigma_seg_accumulate_params* p, void* stream) {
    if (!p) return sigma::fail(SIGMA_OPS_ERR_ARG, "params is NULL");
    if (p->pixels < 0 || p->classes < 1 || p->classes > 65535)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "pixels %lld must not be negative and classes %d be in [1, 65535]", (long long)p->pixels, p->classes);
    if (p->first != 0 && p->first != 1) return sigma::fail(SIGMA_OPS_ERR_ARG, "first must be 0 or 1 (got %d)", p->first);
    if (p->score_plane_stride < p->pixels || p->acc_plane_stride < p->pixels)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "score_plane_stride %lld and acc_plane_stride %lld must be at least pixels (%lld)",
                           (long long)p->score_plane_stride, (long long)p->acc_plane_stride, (long long)p->pixels);
    if (!p->score || !p->acc || !sigma::aligned(p->score, 4) || !sigma::aligned(p->acc, 8))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "score must be a non-NULL 4-byte aligned and acc a non-NULL 8-byte aligned device pointer");
    if (p->pixels == 0) return SIGMA_OPS_OK;
    const bool vec = p->pixels % 4 == 0 && p->score_plane_stride % 4 == 0 && p->acc_plane_stride % 2 == 0 &&
                     sigma::aligned(p->score, 16) && sigma::aligned(p->acc, 16);
    const long n = vec ? p->pixels / 4 : p->pixels;
    long gx = (n + sigma::kSegThreads - 1) / sigma::kSegThreads;
    if (gx > 1024) gx = 1024;
    const dim3 grid((unsigned)gx, (unsigned)p->classes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(sigma::seg_accumulate_kernel<4>, grid, dim3(sigma::kSegThreads), 0, s, p->score, p->acc, (long)p->pixels,
                           (long)p->score_plane_stride, (long)p->acc_plane_stride, (int)p->first);
    else
        hipLaunchKernelGGL(sigma::seg_accumulate_kernel<1>, grid, dim3(sigma::kSegThreads), 0, s, p->score, p->acc, (long)p->pixels,
                           (long)p->score_plane_stride, (long)p->acc_plane_stride, (int)p->first);
    return sigma::launched("seg_accumulate_kernel");
}

int sigma_seg_argmax_confusion(const sigma_seg_confusion_params* p, void* stream) {
    if (!p) return sigma::fail(SIGMA_OPS_ERR_ARG, "params is NULL");
    if (p->pixels < 0 || p->pixels > 2147483647L) return sigma::fail(SIGMA_OPS_ERR_ARG, "pixels %lld must be in [0, 2^31 - 1]", (long long)p->pixels);
    if (p->n_cl < 1 || p->n_cl > 256) return sigma::fail(SIGMA_OPS_ERR_ARG, "n_cl %d must be in [1, 256]", p->n_cl);
    if ((p->gt_elem_size != 1 && p->gt_elem_size != 8) || (p->pred_elem_size != 1 && p->pred_elem_size != 8))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "gt_elem_size %d and pred_elem_size %d must each be 1 or 8", p->gt_elem_size, p->pred_elem_size);
    const bool from_acc = p->acc != nullptr;
    if (from_acc) {
        if (p->classes < 1 || p->classes > 65535 || p->acc_plane_stride < p->pixels || !sigma::aligned(p->acc, 8))
            return sigma::fail(SIGMA_OPS_ERR_ARG, "with acc: classes %d must be in [1, 65535], acc_plane_stride %lld at least pixels (%lld), acc 8-byte aligned",
                               p->classes, (long long)p->acc_plane_stride, (long long)p->pixels);
        if (p->pred_elem_size == 1 && p->classes > 256)      // a uint8 pred could not hold the index
            return sigma::fail(SIGMA_OPS_ERR_ARG, "pred_elem_size 1 cannot hold the index of %d classes", p->classes);
    } else {
        if (p->classes != 0 || !p->pred) return sigma::fail(SIGMA_OPS_ERR_ARG, "without acc: classes must be 0 (got %d) and pred non-NULL", p->classes);
    }
    if (!sigma::aligned(p->pred, (uintptr_t)p->pred_elem_size))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "pred must be aligned to pred_elem_size (%d bytes)", p->pred_elem_size);
    if (!p->gt) {
        if (!from_acc || !p->pred) return sigma::fail(SIGMA_OPS_ERR_ARG, "without gt (arg-max only) acc and pred must be non-NULL");
    } else {
        if (!sigma::aligned(p->gt, (uintptr_t)p->gt_elem_size)) return sigma::fail(SIGMA_OPS_ERR_ARG, "gt must be aligned to gt_elem_size (%d bytes)", p->gt_elem_size);
        if (!p->hist || !p->counts || !sigma::aligned(p->hist, 8) || !sigma::aligned(p->counts, 8))
            return sigma::fail(SIGMA_OPS_ERR_ARG, "with gt: hist and counts must be non-NULL 8-byte aligned device pointers");
    }
    if (p->pixels == 0) return SIGMA_OPS_OK;

    sigma::ConfArgs a{p->acc, (long)p->acc_plane_stride, p->pred, p->gt, reinterpret_cast<unsigned long long*>(p->hist),
                      reinterpret_cast<unsigned long long*>(p->counts), (long)p->pixels, (int)p->classes, (int)p->n_cl};
    const bool lds_hist = (long)p->n_cl * p->n_cl * 4 <= SIGMA_SEG_LDS_HIST_BYTES;
    const int pix = (from_acc && p->pixels % 2 == 0 && p->acc_plane_stride % 2 == 0 && sigma::aligned(p->acc, 16)) ? 2 : 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p->gt_elem_size == 1) {
        if (p->pred_elem_size == 1) sigma::dispatch_confusion<uint8_t, uint8_t>(a, from_acc, lds_hist, pix, s);
        else sigma::dispatch_confusion<uint8_t, int64_t>(a, from_acc, lds_hist, pix, s);
    } else {
        if (p->pred_elem_size == 1) sigma::dispatch_confusion<int64_t, uint8_t>(a, from_acc, lds_hist, pix, s);
        else sigma::dispatch_confusion<int64_t, int64_t>(a, from_acc, lds_hist, pix, s);
    }
    return sigma::launched("seg_confusion_kernel");
}

}  // extern "C"
