// region.hip -- the soft region-overlap losses (Dice, Jaccard, Tversky; include/sigma_region.h) on the row layout of the
// loss family of pointwise.hip: a row of `nc` logits at a pitch of `ld` floats per thread, NC4 = ceil(nc / 4) chunks of 16
// bytes held in registers (nc <= 64).  A translation unit of its own: pointwise.hip's kernels keep their schedule.
//
//   region_sums  SIGMA_CE_BLOCKS workgroups, grid-stride over the rows: lse per row; for a valid row p_c = exp(x_c - lse)
//                joins the thread's P_c, and I_y, Y_y at the label (a select per class: the label indexes registers).  At
//                the end every class is reduced over the wave (the fixed tree of wave_sum), the four waves meet in LDS
//                and are added in wave order; the workgroup stores its slot [I | P | Y | sum nll | count].  No atomics.
//   region_coef  one workgroup of 1024 threads: the slots are added in fp64 in a fixed order (contiguous runs of slots per
//                thread, then the runs in order), then one thread per class forms T_c, A_c, B_c in fp64.
//   region_bwd   one pass: p from the row and the kept lse, g_c = B_c + A_c [c == y], dot = sum p_c g_c,
//                dx_c = G (p_c (g_c - dot) + cw (p_c - [c == y])).  B_c is read with a wave-uniform index (scalar cache),
//                A_y is one gather per row from the same table of at most 129 floats.
// Traffic: 4 bytes per element forward, 8 backward -- that of the cross-entropy kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "ops_host.h"
#include "scan_device.h"
#include "../../include/sigma_region.h"

namespace sigma {
namespace {

constexpr float kNegInf = -INFINITY;
constexpr int kCoefThreads = 1024;

__device__ __forceinline__ void mask_tail(float4& v, int n, float fill) {      // n in [1, 4] columns of v are valid
    if (n < 2) v.y = fill;
    if (n < 3) v.z = fill;
    if (n < 4) v.w = fill;
}

__device__ __forceinline__ float& lane_of(float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

template <int NC4>
__global__ void __launch_bounds__(256)
region_sums_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, long rows, int nc, int ld, long ignore,
                   float* __restrict__ lse, float* __restrict__ partial) {
    constexpr int C = NC4 * 4;
    __shared__ float sh[4][3 * C + 2];
    float P[C], I[C], Y[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { P[c] = 0.0f; I[c] = 0.0f; Y[c] = 0.0f; }
    float nll = 0.0f, cnt = 0.0f;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const float4* __restrict__ xr = reinterpret_cast<const float4*>(logits + r * ld);
        float4 v[NC4];
#pragma unroll
        for (int c = 0; c < NC4; ++c) v[c] = xr[c];
        const long y = labels[r];
        mask_tail(v[NC4 - 1], nc - 4 * (NC4 - 1), kNegInf);          // columns [nc, 4 NC4): p = 0
        float m = kNegInf;
#pragma unroll
        for (int c = 0; c < NC4; ++c) m = fmaxf(m, fmaxf(fmaxf(v[c].x, v[c].y), fmaxf(v[c].z, v[c].w)));
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < NC4; ++c) s += (__expf(v[c].x - m) + __expf(v[c].y - m)) + (__expf(v[c].z - m) + __expf(v[c].w - m));
        const float l = m + __logf(s);
        lse[r] = l;
        if (y != ignore && y >= 0 && y < nc) {
            float xy = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float x = lane_of(v[c >> 2], c & 3);
                const float p = __expf(x - l);
                const bool hit = y == c;
                P[c] += p;
                I[c] += hit ? p : 0.0f;
                Y[c] += hit ? 1.0f : 0.0f;
                xy = hit ? x : xy;
            }
            nll += l - xy;
            cnt += 1.0f;
        }
    }
    // every class over the wave, then the four waves in wave order
    const int w = threadIdx.x >> 6;
    const bool first = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float ti = wave_sum(I[c]), tp = wave_sum(P[c]), ty = wave_sum(Y[c]);
        if (first && c < nc) { sh[w][c] = ti; sh[w][nc + c] = tp; sh[w][2 * nc + c] = ty; }
    }
    const float tn = wave_sum(nll), tc = wave_sum(cnt);
    if (first) { sh[w][3 * nc] = tn; sh[w][3 * nc + 1] = tc; }
    __syncthreads();
    const int ncol = 3 * nc + 2;
    for (int j = threadIdx.x; j < ncol; j += 256)
        partial[(long)blockIdx.x * ncol + j] = ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
}

// `cols` = the power of two >= 3 nc + 2 (<= 256); thread t adds the run of slots [part per, (part + 1) per) of column
// t % cols, part = t / cols; then one thread per column adds the runs in order.  fp64 throughout.
__global__ void __launch_bounds__(kCoefThreads)
region_coef_kernel(const float* __restrict__ partial, int nc, double a, double b, double s, double rw, double cw,
                   float* __restrict__ loss, float* __restrict__ terms, float* __restrict__ coef, float* __restrict__ sums) {
    __shared__ double part[kCoefThreads];
    __shared__ double tot[256];
    __shared__ double miss[64];
    __shared__ int present[64];
    const int ncol = 3 * nc + 2;
    int cols = 8;
    while (cols < ncol) cols <<= 1;
    const int parts = kCoefThreads / cols, per = SIGMA_CE_BLOCKS / parts;
    const int col = threadIdx.x & (cols - 1), run = threadIdx.x / cols;
    double acc = 0.0;
    if (col < ncol) {
        const float* __restrict__ q = partial + (long)run * per * ncol + col;
#pragma unroll 16
        for (int k = 0; k < per; ++k) acc += (double)q[(long)k * ncol];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < ncol) {
        double t = 0.0;
        for (int i = 0; i < parts; ++i) t += part[i * cols + threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    const int c = threadIdx.x;
    double N = 0.0, D = 1.0;
    bool in = false;
    if (c < nc) {
        const double Ic = tot[c], Pc = tot[nc + c], Yc = tot[2 * nc + c];
        sums[c] = (float)Ic; sums[nc + c] = (float)Pc; sums[2 * nc + c] = (float)Yc;
        in = Yc > 0.0;
        if (in) {
            N = Ic + s;
            D = (1.0 - a - b) * Ic + a * Pc + b * Yc + s;
        }
        present[c] = in ? 1 : 0;
        miss[c] = in ? 1.0 - N / D : 0.0;
    }
    __syncthreads();
    if (c < nc) {
        int k = 0;
        for (int i = 0; i < nc; ++i) k += present[i];
        const double f = in ? rw / (double)k : 0.0;
        coef[c] = in ? (float)(-f * (D - (1.0 - a - b) * N) / (D * D)) : 0.0f;
        coef[nc + c] = in ? (float)(f * a * N / (D * D)) : 0.0f;
        if (c == 0) {
            double region = 0.0;
            for (int i = 0; i < nc; ++i) region += miss[i];
            region = k > 0 ? region / (double)k : 0.0;
            const double n = tot[3 * nc + 1];
            const double ce = n > 0.0 ? tot[3 * nc] / n : 0.0;
            loss[0] = (float)(rw * region + cw * ce);
            terms[0] = (float)region;
            terms[1] = (float)ce;
            coef[2 * nc] = n > 0.0 ? (float)(cw / n) : 0.0f;
        }
    }
}

template <int NC4>
__global__ void __launch_bounds__(256)
region_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ lse,
                  const float* __restrict__ coef, const float* __restrict__ scale, long rows, int nc, int ld, long ignore,
                  float* __restrict__ dlogits) {
    constexpr int C = NC4 * 4;
    const float G = scale[0], cw = coef[2 * nc];
    const long stride = (long)gridDim.x * blockDim.x;
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const float4* __restrict__ xr = reinterpret_cast<const float4*>(logits + r * ld);
        float4* __restrict__ dr = reinterpret_cast<float4*>(dlogits + r * ld);
        float4 v[NC4];
#pragma unroll
        for (int c = 0; c < NC4; ++c) v[c] = xr[c];
        const long y = labels[r];
        const float l = lse[r];
        const bool on = y != ignore && y >= 0 && y < nc;
        const float ay = coef[on ? y : 0];
        mask_tail(v[NC4 - 1], nc - 4 * (NC4 - 1), kNegInf);
        float dot = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float& x = lane_of(v[c >> 2], c & 3);
            const float p = __expf(x - l);
            const float g = coef[nc + (c < nc ? c : nc - 1)] + (y == c ? ay : 0.0f);
            dot += p * g;
            x = p;                                                     // the row's registers hold p from here on
        }
#pragma unroll
        for (int c = 0; c < NC4; ++c) {
            float4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = 4 * c + i;
                const float p = lane_of(v[c], i);
                const float g = coef[nc + (k < nc ? k : nc - 1)] + (y == k ? ay : 0.0f);
                const float d = G * (p * (g - dot) + cw * (p - (y == k ? 1.0f : 0.0f)));
                lane_of(o, i) = (on && k < nc) ? d : 0.0f;             // ignored rows and the pad: zeros chosen by index
            }
            dr[c] = o;
        }
        for (int c = NC4; c < (ld >> 2); ++c) dr[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// NC4 = ceil(classes / 4) chunks held in registers, classes <= 64
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

unsigned bwd_grid(long rows) {
    long b = (rows + 255) / 256;
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}

int64_t workspace_bytes(int classes) { return (int64_t)SIGMA_CE_BLOCKS * (3 * classes + 2) * (int64_t)sizeof(float); }

// what all three entry points refuse on the values alone
int check_values(const sigma_region_params* p, int code) {
    if (!p) return fail(code, "params is NULL");
    if (p->classes < 1 || p->classes > 64) return fail(code, "classes %d must be in [1, 64]", p->classes);
    if (p->ld % 4 != 0 || p->ld < p->classes) return fail(code, "ld %d must be a multiple of 4, at least classes %d", p->ld, p->classes);
    if (p->rows < 0) return fail(code, "rows %lld must not be negative", (long long)p->rows);
    if (!(p->beta > 0.0)) return fail(code, "beta %g must be positive", p->beta);                // NaN fails each
    if (!(p->alpha >= 0.0)) return fail(code, "alpha %g must not be negative", p->alpha);
    if (!(p->smooth >= 0.0)) return fail(code, "smooth %g must not be negative", p->smooth);
    if (!(p->region_weight >= 0.0)) return fail(code, "region_weight %g must not be negative", p->region_weight);
    if (!(p->ce_weight >= 0.0)) return fail(code, "ce_weight %g must not be negative", p->ce_weight);
    return SIGMA_OPS_OK;
}

// the pointers both directions read
int check_rows(const sigma_region_params* p) {
    if (p->rows > 0) {
        if (!p->logits) return fail(SIGMA_OPS_ERR_ARG, "logits is NULL");
        if (!p->labels) return fail(SIGMA_OPS_ERR_ARG, "labels is NULL");
        if (!p->lse) return fail(SIGMA_OPS_ERR_ARG, "lse is NULL");
    }
    if (!p->coef) return fail(SIGMA_OPS_ERR_ARG, "coef is NULL");
    if (!aligned(p->logits, 16)) return fail(SIGMA_OPS_ERR_ARG, "alignment: logits %p needs 16 bytes", (const void*)p->logits);
    if (!aligned(p->labels, 8)) return fail(SIGMA_OPS_ERR_ARG, "alignment: labels %p needs 8 bytes", (const void*)p->labels);
    if (!aligned(p->lse, 4) || !aligned(p->coef, 4))
        return fail(SIGMA_OPS_ERR_ARG, "alignment: lse %p and coef %p need 4 bytes", (const void*)p->lse, (const void*)p->coef);
    return SIGMA_OPS_OK;
}

}  // namespace
}  // namespace sigma

extern "C" {

int64_t sigma_region_loss_workspace_bytes(const sigma_region_params* p) {
    if (sigma::check_values(p, -1)) return -1;
    return sigma::workspace_bytes(p->classes);
}

int sigma_region_loss_fwd(const sigma_region_params* p, void* stream) {
    if (const int rc = sigma::check_values(p, SIGMA_OPS_ERR_ARG)) return rc;
    if (const int rc = sigma::check_rows(p)) return rc;
    if (!p->loss) return sigma::fail(SIGMA_OPS_ERR_ARG, "loss is NULL");
    if (!p->terms) return sigma::fail(SIGMA_OPS_ERR_ARG, "terms is NULL");
    if (!p->sums) return sigma::fail(SIGMA_OPS_ERR_ARG, "sums is NULL");
    if (!sigma::aligned(p->loss, 4) || !sigma::aligned(p->terms, 4) || !sigma::aligned(p->sums, 4))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "alignment: loss %p, terms %p and sums %p need 4 bytes", (const void*)p->loss,
                           (const void*)p->terms, (const void*)p->sums);
    if (!p->workspace || !sigma::aligned(p->workspace, 4) || p->workspace_bytes < sigma::workspace_bytes(p->classes))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "a 4-byte aligned workspace of %lld bytes is required (got %p, %lld bytes)",
                           (long long)sigma::workspace_bytes(p->classes), p->workspace, (long long)p->workspace_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* partial = static_cast<float*>(p->workspace);
    // every workgroup writes its slot, rows or not: the second kernel adds all of them
    sigma::dispatch_nc4((p->classes + 3) / 4, [&](auto n) {
        hipLaunchKernelGGL(sigma::region_sums_kernel<decltype(n)::value>, dim3(SIGMA_CE_BLOCKS), dim3(256), 0, st, p->logits, p->labels,
                           (long)p->rows, (int)p->classes, (int)p->ld, (long)p->ignore_index, p->lse, partial);
    });
    if (const int rc = sigma::launched("region_sums_kernel")) return rc;
    hipLaunchKernelGGL(sigma::region_coef_kernel, dim3(1), dim3(sigma::kCoefThreads), 0, st, partial, (int)p->classes, p->alpha, p->beta,
                       p->smooth, p->region_weight, p->ce_weight, p->loss, p->terms, p->coef, p->sums);
    return sigma::launched("region_coef_kernel");
}

int sigma_region_loss_bwd(const sigma_region_params* p, void* stream) {
    if (const int rc = sigma::check_values(p, SIGMA_OPS_ERR_ARG)) return rc;
    if (const int rc = sigma::check_rows(p)) return rc;
    if (!p->scale) return sigma::fail(SIGMA_OPS_ERR_ARG, "scale is NULL");
    if (!sigma::aligned(p->scale, 4)) return sigma::fail(SIGMA_OPS_ERR_ARG, "alignment: scale %p needs 4 bytes", (const void*)p->scale);
    if (p->rows > 0 && !p->dlogits) return sigma::fail(SIGMA_OPS_ERR_ARG, "dlogits is NULL");
    if (!sigma::aligned(p->dlogits, 16)) return sigma::fail(SIGMA_OPS_ERR_ARG, "alignment: dlogits %p needs 16 bytes", (const void*)p->dlogits);
    if (p->rows == 0) return SIGMA_OPS_OK;
    sigma::dispatch_nc4((p->classes + 3) / 4, [&](auto n) {
        hipLaunchKernelGGL(sigma::region_bwd_kernel<decltype(n)::value>, dim3(sigma::bwd_grid((long)p->rows)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), p->logits, p->labels, p->lse, p->coef, p->scale, (long)p->rows,
                           (int)p->classes, (int)p->ld, (long)p->ignore_index, p->dlogits);
    });
    return sigma::launched("region_bwd_kernel");
}

}  // extern "C"
