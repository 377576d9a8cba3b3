// distill.hip -- the distillation loss (temperature KL against a teacher + cross entropy; include/sigma_distill.h) on the row
// layout of the loss family of pointwise.hip, as region.hip: one thread per row, NC4 = ceil(nc / 4) chunks of 16 bytes held
// in registers (nc <= 64) -- here two rows per thread, the student's at a pitch of `ld` floats and the teacher's at `ldt`.
//
//   distill_sums  SIGMA_CE_BLOCKS workgroups, grid-stride over the rows: lse(x), lse(x k), lse(t k) per row (k = 1 / T as a
//                 float); kl_r = sum_c [q_c > 0] q_c (lp(t)_c - lp(x)_c) joins the thread's sum for the rows of S and
//                 lse(x) - x_y for the valid rows, each with its count.  At the end the four sums are reduced over the wave
//                 (the fixed tree of wave_sum), the four waves meet in LDS and are added in wave order; the workgroup stores
//                 its slot [sum kl | |S| | sum nll | n].  No atomics.
//   distill_coef  one workgroup of 1024 threads adds the slots in fp64 in a fixed order (runs of 4 slots, 16 runs, 16 groups)
//                 and writes the loss, both terms and the two coefficients.
//   distill_bwd   one pass: p, q and P1 from the two rows and the kept lse,
//                 dx_c = G ([r in S] coef[0] (p_c - q_c) + [r valid] coef[1] (P1_c - [c == y])).
// lp(v)_c = v_c k - lse(v k) is formed by `logp` from the lse of `row_lse` for the student and the teacher alike (the build
// has no fp contraction), so equal bits in give equal bits out: kl_r == 0 and p_c - q_c == 0 for a teacher equal to the student.
// Traffic: 8 bytes per element forward, 12 backward.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "ops_host.h"
#include "scan_device.h"
#include "../../include/sigma_distill.h"

namespace sigma {
namespace {

constexpr float kNegInf = -INFINITY;
constexpr int kCoefThreads = 1024;
static_assert(SIGMA_CE_BLOCKS == 1024, "distill_coef_kernel adds 256 runs of 4 slots");

__device__ __forceinline__ void mask_tail(float4& v, int n, float fill) {      // n in [1, 4] columns of v are valid
    if (n < 2) v.y = fill;
    if (n < 3) v.z = fill;
    if (n < 4) v.w = fill;
}

__device__ __forceinline__ float& lane_of(float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
__device__ __forceinline__ float lane_of(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// lse of the row v scaled by k > 0 (k = 1.0f literally: the row itself), the register form of pointwise.hip
template <int NC4>
__device__ __forceinline__ float row_lse(const float4 (&v)[NC4], float k) {
    float m = kNegInf;
#pragma unroll
    for (int c = 0; c < NC4; ++c) m = fmaxf(m, fmaxf(fmaxf(v[c].x * k, v[c].y * k), fmaxf(v[c].z * k, v[c].w * k)));
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < NC4; ++c)
        s += (__expf(v[c].x * k - m) + __expf(v[c].y * k - m)) + (__expf(v[c].z * k - m) + __expf(v[c].w * k - m));
    return m + __logf(s);
}

// the log-probability of one column at temperature 1 / k, from the lse of row_lse(., k)
__device__ __forceinline__ float logp(float v, float k, float l) { return v * k - l; }

__device__ __forceinline__ float kl_term(float x, float t, float k, float lx, float lt) {
    const float a = logp(t, k, lt), b = logp(x, k, lx);
    const float q = __expf(a);
    return q > 0.0f ? q * (a - b) : 0.0f;                 // q == 0: exactly 0, whatever a - b is (-inf - -inf in the pad)
}

template <int NC4>
__global__ void __launch_bounds__(256)
distill_sums_kernel(const float* __restrict__ logits, const float* __restrict__ teacher, const int64_t* __restrict__ labels, long rows,
                    int nc, int ld, int ldt, int kd_all, long ignore, float k, float* __restrict__ lse, float* __restrict__ partial) {
    constexpr int C = NC4 * 4;
    __shared__ float sh[4][4];
    float kl = 0.0f, ns = 0.0f, nll = 0.0f, cnt = 0.0f;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const float4* __restrict__ xr = reinterpret_cast<const float4*>(logits + r * ld);
        const float4* __restrict__ tr = reinterpret_cast<const float4*>(teacher + r * ldt);
        float4 v[NC4], u[NC4];
#pragma unroll
        for (int c = 0; c < NC4; ++c) v[c] = xr[c];
#pragma unroll
        for (int c = 0; c < NC4; ++c) u[c] = tr[c];
        const long y = labels[r];
        mask_tail(v[NC4 - 1], nc - 4 * (NC4 - 1), kNegInf);          // columns [nc, 4 NC4): p = q = 0
        mask_tail(u[NC4 - 1], nc - 4 * (NC4 - 1), kNegInf);
        const float l1 = row_lse<NC4>(v, 1.0f), lx = row_lse<NC4>(v, k), lt = row_lse<NC4>(u, k);
        lse[3 * r] = l1;
        lse[3 * r + 1] = lx;
        lse[3 * r + 2] = lt;
        const bool valid = y != ignore && y >= 0 && y < nc;
        if (valid || kd_all) {
            float t = 0.0f;
#pragma unroll
            for (int c = 0; c < NC4; ++c)
                t += (kl_term(v[c].x, u[c].x, k, lx, lt) + kl_term(v[c].y, u[c].y, k, lx, lt))
                   + (kl_term(v[c].z, u[c].z, k, lx, lt) + kl_term(v[c].w, u[c].w, k, lx, lt));
            kl += t;
            ns += 1.0f;
        }
        if (valid) {
            float xy = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) xy = y == c ? lane_of(v[c >> 2], c & 3) : xy;
            nll += l1 - xy;
            cnt += 1.0f;
        }
    }
    // over the wave, then the four waves in wave order
    const int w = threadIdx.x >> 6;
    const float t0 = wave_sum(kl), t1 = wave_sum(ns), t2 = wave_sum(nll), t3 = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) { sh[w][0] = t0; sh[w][1] = t1; sh[w][2] = t2; sh[w][3] = t3; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int j = threadIdx.x;
        partial[(long)blockIdx.x * 4 + j] = ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
    }
}

// thread t adds the run of slots [4 (t / 4), 4 (t / 4) + 4) of column t % 4; 64 threads add 16 runs each in order; one
// thread adds the 16 groups in order.  fp64 throughout.
__global__ void __launch_bounds__(kCoefThreads)
distill_coef_kernel(const float* __restrict__ partial, double T, double kw, double cw, float* __restrict__ loss,
                    float* __restrict__ terms, float* __restrict__ coef) {
    __shared__ double run[kCoefThreads];
    __shared__ double group[64];
    const int t = threadIdx.x, col = t & 3;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc += (double)partial[(long)((t >> 2) * 4 + i) * 4 + col];
    run[t] = acc;
    __syncthreads();
    if (t < 64) {
        double s = 0.0;
        for (int i = 0; i < 16; ++i) s += run[(((t >> 2) * 16 + i) << 2) + col];
        group[t] = s;
    }
    __syncthreads();
    if (t == 0) {
        double tot[4];
        for (int c = 0; c < 4; ++c) {
            double s = 0.0;
            for (int h = 0; h < 16; ++h) s += group[h * 4 + c];
            tot[c] = s;
        }
        const double S = tot[1], n = tot[3];
        const double kd = S > 0.0 ? T * T * tot[0] / S : 0.0;
        const double ce = n > 0.0 ? tot[2] / n : 0.0;
        loss[0] = (float)(kw * kd + cw * ce);
        terms[0] = (float)kd;
        terms[1] = (float)ce;
        coef[0] = S > 0.0 ? (float)(kw * T / S) : 0.0f;
        coef[1] = n > 0.0 ? (float)(cw / n) : 0.0f;
    }
}

template <int NC4>
__global__ void __launch_bounds__(256)
distill_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ teacher, const int64_t* __restrict__ labels,
                   const float* __restrict__ lse, const float* __restrict__ coef, const float* __restrict__ scale, long rows, int nc,
                   int ld, int ldt, int kd_all, long ignore, float k, float* __restrict__ dlogits) {
    const float G = scale[0], ck = coef[0], cc = coef[1];
    const long stride = (long)gridDim.x * blockDim.x;
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const float4* __restrict__ xr = reinterpret_cast<const float4*>(logits + r * ld);
        const float4* __restrict__ tr = reinterpret_cast<const float4*>(teacher + r * ldt);
        float4* __restrict__ dr = reinterpret_cast<float4*>(dlogits + r * ld);
        float4 v[NC4], u[NC4];
#pragma unroll
        for (int c = 0; c < NC4; ++c) v[c] = xr[c];
#pragma unroll
        for (int c = 0; c < NC4; ++c) u[c] = tr[c];
        const long y = labels[r];
        const float l1 = lse[3 * r], lx = lse[3 * r + 1], lt = lse[3 * r + 2];
        const bool valid = y != ignore && y >= 0 && y < nc;
        const bool in_s = valid || kd_all;
        const int yi = valid ? (int)y : -1;
        mask_tail(v[NC4 - 1], nc - 4 * (NC4 - 1), kNegInf);
        mask_tail(u[NC4 - 1], nc - 4 * (NC4 - 1), kNegInf);
#pragma unroll
        for (int c = 0; c < NC4; ++c) {
            float4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = 4 * c + i;
                const float x = lane_of(v[c], i), t = lane_of(u[c], i);
                const float p = __expf(logp(x, k, lx)), q = __expf(logp(t, k, lt)), p1 = __expf(x - l1);
                const float dk = in_s ? ck * (p - q) : 0.0f;
                const float dc = valid ? cc * (p1 - (yi == j ? 1.0f : 0.0f)) : 0.0f;
                // rows outside both sets and the pad (the last chunk alone can reach it): zeros chosen by index
                lane_of(o, i) = (in_s && (c < NC4 - 1 || j < nc)) ? G * (dk + dc) : 0.0f;
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

constexpr int64_t kWorkspaceBytes = (int64_t)SIGMA_CE_BLOCKS * 4 * (int64_t)sizeof(float);

// what all three entry points refuse on the values alone
int check_values(const sigma_distill_params* p, int code) {
    if (!p) return fail(code, "params is NULL");
    if (p->classes < 1 || p->classes > 64) return fail(code, "classes %d must be in [1, 64]", p->classes);
    if (p->ld % 4 != 0 || p->ld < p->classes) return fail(code, "ld %d must be a multiple of 4, at least classes %d", p->ld, p->classes);
    if (p->ld_t % 4 != 0 || p->ld_t < p->classes)
        return fail(code, "ld_t %d must be a multiple of 4, at least classes %d", p->ld_t, p->classes);
    if (p->rows < 0) return fail(code, "rows %lld must not be negative", (long long)p->rows);
    if (!(p->temperature > 0.0)) return fail(code, "temperature %g must be positive", p->temperature);      // NaN fails each
    if (!(p->kd_weight >= 0.0)) return fail(code, "kd_weight %g must not be negative", p->kd_weight);
    if (!(p->ce_weight >= 0.0)) return fail(code, "ce_weight %g must not be negative", p->ce_weight);
    return SIGMA_OPS_OK;
}

// the pointers both directions read
int check_rows(const sigma_distill_params* p) {
    if (p->rows > 0) {
        if (!p->logits) return fail(SIGMA_OPS_ERR_ARG, "logits is NULL");
        if (!p->teacher) return fail(SIGMA_OPS_ERR_ARG, "teacher is NULL");
        if (!p->labels) return fail(SIGMA_OPS_ERR_ARG, "labels is NULL");
        if (!p->lse) return fail(SIGMA_OPS_ERR_ARG, "lse is NULL");
    }
    if (!p->coef) return fail(SIGMA_OPS_ERR_ARG, "coef is NULL");
    if (!aligned(p->logits, 16)) return fail(SIGMA_OPS_ERR_ARG, "alignment: logits %p needs 16 bytes", (const void*)p->logits);
    if (!aligned(p->teacher, 16)) return fail(SIGMA_OPS_ERR_ARG, "alignment: teacher %p needs 16 bytes", (const void*)p->teacher);
    if (!aligned(p->labels, 8)) return fail(SIGMA_OPS_ERR_ARG, "alignment: labels %p needs 8 bytes", (const void*)p->labels);
    if (!aligned(p->lse, 4)) return fail(SIGMA_OPS_ERR_ARG, "alignment: lse %p needs 4 bytes", (const void*)p->lse);
    if (!aligned(p->coef, 4)) return fail(SIGMA_OPS_ERR_ARG, "alignment: coef %p needs 4 bytes", (const void*)p->coef);
    return SIGMA_OPS_OK;
}

}  // namespace
}  // namespace sigma

extern "C" {

int64_t sigma_distill_loss_workspace_bytes(const sigma_distill_params* p) {
    if (sigma::check_values(p, -1)) return -1;
    return sigma::kWorkspaceBytes;
}

int sigma_distill_loss_fwd(const sigma_distill_params* p, void* stream) {
    if (const int rc = sigma::check_values(p, SIGMA_OPS_ERR_ARG)) return rc;
    if (const int rc = sigma::check_rows(p)) return rc;
    if (!p->loss) return sigma::fail(SIGMA_OPS_ERR_ARG, "loss is NULL");
    if (!p->terms) return sigma::fail(SIGMA_OPS_ERR_ARG, "terms is NULL");
    if (!sigma::aligned(p->loss, 4)) return sigma::fail(SIGMA_OPS_ERR_ARG, "alignment: loss %p needs 4 bytes", (const void*)p->loss);
    if (!sigma::aligned(p->terms, 4)) return sigma::fail(SIGMA_OPS_ERR_ARG, "alignment: terms %p needs 4 bytes", (const void*)p->terms);
    if (!p->workspace || !sigma::aligned(p->workspace, 4) || p->workspace_bytes < sigma::kWorkspaceBytes)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "a 4-byte aligned workspace of %lld bytes is required (got %p, %lld bytes)",
                           (long long)sigma::kWorkspaceBytes, p->workspace, (long long)p->workspace_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* partial = static_cast<float*>(p->workspace);
    const float k = (float)(1.0 / p->temperature);
    // every workgroup writes its slot, rows or not: the second kernel adds all of them
    sigma::dispatch_nc4((p->classes + 3) / 4, [&](auto n) {
        hipLaunchKernelGGL(sigma::distill_sums_kernel<decltype(n)::value>, dim3(SIGMA_CE_BLOCKS), dim3(256), 0, st, p->logits, p->teacher,
                           p->labels, (long)p->rows, (int)p->classes, (int)p->ld, (int)p->ld_t, (int)(p->kd_all != 0),
                           (long)p->ignore_index, k, p->lse, partial);
    });
    if (const int rc = sigma::launched("distill_sums_kernel")) return rc;
    hipLaunchKernelGGL(sigma::distill_coef_kernel, dim3(1), dim3(sigma::kCoefThreads), 0, st, partial, p->temperature, p->kd_weight,
                       p->ce_weight, p->loss, p->terms, p->coef);
    return sigma::launched("distill_coef_kernel");
}

int sigma_distill_loss_bwd(const sigma_distill_params* p, void* stream) {
    if (const int rc = sigma::check_values(p, SIGMA_OPS_ERR_ARG)) return rc;
    if (const int rc = sigma::check_rows(p)) return rc;
    if (!p->scale) return sigma::fail(SIGMA_OPS_ERR_ARG, "scale is NULL");
    if (!sigma::aligned(p->scale, 4)) return sigma::fail(SIGMA_OPS_ERR_ARG, "alignment: scale %p needs 4 bytes", (const void*)p->scale);
    if (p->rows > 0 && !p->dlogits) return sigma::fail(SIGMA_OPS_ERR_ARG, "dlogits is NULL");
    if (!sigma::aligned(p->dlogits, 16)) return sigma::fail(SIGMA_OPS_ERR_ARG, "alignment: dlogits %p needs 16 bytes", (const void*)p->dlogits);
    if (p->rows == 0) return SIGMA_OPS_OK;
    const float k = (float)(1.0 / p->temperature);
    sigma::dispatch_nc4((p->classes + 3) / 4, [&](auto n) {
        hipLaunchKernelGGL(sigma::distill_bwd_kernel<decltype(n)::value>, dim3(sigma::bwd_grid((long)p->rows)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), p->logits, p->teacher, p->labels, p->lse, p->coef, p->scale, (long)p->rows,
                           (int)p->classes, (int)p->ld, (int)p->ld_t, (int)(p->kd_all != 0), (long)p->ignore_index, k, p->dlogits);
    });
    return sigma::launched("distill_bwd_kernel");
}

}  // extern "C"
