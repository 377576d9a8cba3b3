// dwconv.hip -- depthwise 3x3 convolution + SiLU of SS2D, fused with the CrossScan layout step.
//
// Reference (models/encoders/vmamba.py:1071-1072, 683-691):
//     x = x.permute(0, 3, 1, 2).contiguous();  x = self.act(self.conv2d(x))       # Conv2d(d, d, 3, pad 1, groups=d) + SiLU
// followed by CrossScan's four permuted copies (vmamba.py:80-98).  On MI355X all of it is HBM-bound
// stencil / transpose work, so it is one pass: read the (B, d, H, W) plane once, write the activation in
// BOTH memory orders the scan kernels consume (row-major, and column-major through a transposed LDS tile so
// that both stores are coalesced).  MIOpen serves this shape with its "naive_conv" fallbacks.
//
//   fwd :  y = silu(conv3x3(x) + bias)                 -> out[b, 0, c, h*W + w],  out[b, 1, c, w*H + h]
//   bwd1:  gpre = (g[b,0,c,h*W+w] + g[b,1,c,w*H+h]) * silu'(conv3x3(x) + bias)    (pre-activation recomputed)
//          dW[c, :, :] += sum gpre * x(shifted),  dbias[c] += sum gpre             (block reduce + one atomic each)
//   bwd2:  dx = correlate(gpre, W)                                                  (transposed stencil)
//
// Every kernel works on a RECT of one (batch, channel) plane: `th` rows x `tw` columns (tw % 4 == 0).  The rect is staged
// once, with its one-pixel halo, into a bordered LDS image (16-byte loads where the plane allows them, zeros outside the
// plane); a thread then owns RUNS of four consecutive pixels of a row and reads the 3 x 6 window of a run once: 18 LDS
// words per four pixels where the per-pixel kernels fetched 36 (from LDS, or as 36 four-byte global loads).  Rows and
// columns of a thread's items are carried from item to item (Walk), set up with two float reciprocals per thread and
// loop: no integer division per pixel.  The column-major order goes through a transposed LDS tile [column][row] (odd
// pitch) whose global side is contiguous along h.  A workgroup has about one thread per three runs (threads_for).
//
//   forward, any plane            : strips of <= 32 rows x <= 128 columns, one workgroup each (dwconv_silu_fwd_kernel)
//   backward, plane below 48 KiB  : ONE workgroup per plane, gpre stays in LDS between the two stencils and p->gpre is not
//                                   touched (dwconv_silu_bwd_plane_kernel)
//   backward, larger planes       : the same strips, two launches with gpre through memory (dwconv_silu_bwd1_kernel,
//                                   dwconv_bwd2_kernel)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ops_host.h"
#include "scan_device.h"

namespace sigma {

namespace {

constexpr int kThreads = 256;       // most threads of a workgroup; a rect of few runs takes fewer (threads_for)
constexpr int kTile = 32;          // rows / columns of the tile grid the deterministic workspace is sized by (sigma_ops.h)
constexpr int kStripTiles = 4;     // a strip spans up to 4 x 32 columns
constexpr int kStripRuns = 4;      // most runs of a thread in a strip: 32 rows x 32 runs / 256 threads
constexpr int kPlaneRuns = 6;      // most runs of a thread in the whole-plane backward (host: plane_rect_lds_bytes)

struct DwArgs {
    const float* x; const float* w; const float* bias;
    float* out2;            // fwd: (B, 2, d, L)
    const float* g2;        // bwd1: (B, 2, d, L)
    float* gpre;            // bwd1 out / bwd2 in: (B, d, H, W)
    float* dw; float* dbias;   // (d, 9), (d): accumulated
    float* dx;              // bwd2 out: (B, d, H, W)
    int B, d, H, W, orders;
    long x_bs, x_cs;        // plane (b, c) of x / dx at b * x_bs + c * x_cs floats (packed: d * L, L)
    float* part;            // deterministic mode: [b * strips + strip][d][10] per-workgroup sums (dW[9], dbias), else NULL
    int vec;                // W % 4 == 0 and every plane the launch touches starts on a 16-byte boundary: 16-byte global accesses
    int th, m, nblk, spp;   // strips: rows per strip, 32-column tiles per strip, strips per row of strips and per plane
    int compact;            // whole-plane backward of a plane too narrow for the bordered 16-byte image (compact body)
};

// the 10 per-channel sums of a workgroup (threads 0..9): one atomic each, or (DET) a plain store into the workgroup's slot
template <bool DET>
__device__ __forceinline__ void dw_leave(const DwArgs& a, int c, int slot, int k, float s) {
    if constexpr (DET) {
        a.part[((long)slot * a.d + c) * 10 + k] = s;
    } else {
        (void)slot;
        if (k < 9) atomicAdd(a.dw + c * 9 + k, s);
        else if (a.dbias) atomicAdd(a.dbias + c, s);
    }
}

// first element of plane `plane_id` = b * d + c of x / dx (the other tensors are packed)
__device__ __forceinline__ long x_plane_offset(const DwArgs& a, int plane_id) {
    const int b = plane_id / a.d, c = plane_id - b * a.d;
    return (long)b * a.x_bs + (long)c * a.x_cs;
}

__device__ __forceinline__ float sigmoidf_fast(float v) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-v * 1.4426950408889634f));
}

// DPP row / bcast adds (scan_device.h wave_sum) instead of six ds_bpermute per sum: ten sums per workgroup
__device__ __forceinline__ float wave_sum_shfl(float v) { return wave_sum(v); }

// all LDS of these kernels is dynamic, so that its base stays 16-byte aligned for the b128 accesses
extern __shared__ __attribute__((aligned(16))) float dw_smem[];

// i / n for 0 <= i <= 256 and 1 <= n < 2^20 without the integer-division sequence: the float quotient is within one of it
__device__ __forceinline__ int small_div(int i, int n) {
    int q = (int)((float)i * __builtin_amdgcn_rcpf((float)n));
    const int r = i - q * n;
    q += r >= n ? 1 : 0;
    q -= r < 0 ? 1 : 0;
    return q;
}

// (q, r) = divmod(i, n) for i = threadIdx.x, carried over i += blockDim.x
struct Walk {
    int q, r, dq, dr, n;
    __device__ __forceinline__ Walk(int n_) : n(n_) {
        q = small_div((int)threadIdx.x, n_); r = (int)threadIdx.x - q * n_;
        dq = small_div((int)blockDim.x, n_); dr = (int)blockDim.x - dq * n_;
    }
    __device__ __forceinline__ void step() { q += dq; r += dr; if (r >= n) { r -= n; ++q; } }
};

// th x tw window of a plane at (h0, w0), tw % 4 == 0; vr x vc of it lies inside the plane
struct Rect { int h0, w0, th, tw, vr, vc; };

__device__ __forceinline__ int img_floats(const Rect& t) { return (t.th + 2) * (t.tw + 8); }
__device__ __forceinline__ int tr_floats(const Rect& t) { return (t.tw * (t.th | 1) + 3) & ~3; }

__device__ __forceinline__ Rect strip_rect(const DwArgs& a, int strip_id) {
    Rect t;
    const int sy = a.nblk == 1 ? strip_id : strip_id / a.nblk, bx = strip_id - sy * a.nblk;
    t.h0 = sy * a.th; t.w0 = bx * kTile * a.m;
    t.th = a.th; t.vr = min(a.th, a.H - t.h0);
    t.tw = min(kTile * a.m, (a.W - t.w0 + 3) & ~3); t.vc = min(t.tw, a.W - t.w0);
    return t;
}

// bordered image of a rect: (th + 2) rows of pitch tw + 8, plane pixel (h0 + hl, w0 + wl) at [(hl + 1) * pitch + 4 + wl];
// the halo (a group of four on either side, a row above and below) holds the neighbouring pixels, 0 outside the plane.
// Every group of four is one item; a thread's loads of four items are issued before their LDS stores.
__device__ __forceinline__ void stage_image(float* __restrict__ img, const float* __restrict__ plane, int H, int W, const Rect& t, bool vec) {
    const int G = (t.tw >> 2) + 2, P = t.tw + 8, items = (t.th + 2) * G, nt = blockDim.x;
    Walk k(G);                             // q = image row, r = group
    for (int i = threadIdx.x; i < items; i += 4 * nt) {
        float4 v[4];
        int off[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            off[u] = -1;
            if (i + u * nt < items) {
                off[u] = k.q * P + 4 * k.r;
                const int h = t.h0 + k.q - 1, w = t.w0 + 4 * (k.r - 1);
                if (h >= 0 && h < H) {
                    const long s = (long)h * W + w;
                    if (vec) {
                        if (w >= 0 && w < W) v[u] = *reinterpret_cast<const float4*>(plane + s);
                    } else {
                        if (w >= 0 && w < W) v[u].x = plane[s];
                        if (w + 1 >= 0 && w + 1 < W) v[u].y = plane[s + 1];
                        if (w + 2 >= 0 && w + 2 < W) v[u].z = plane[s + 2];
                        if (w + 3 >= 0 && w + 3 < W) v[u].w = plane[s + 3];
                    }
                }
            }
            k.step();
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (off[u] >= 0) *reinterpret_cast<float4*>(img + off[u]) = v[u];
    }
}

// transposed tile of a rect: [wl * (th | 1) + hl] = the column-major plane's (w0 + wl) * H + h0 + hl, read along h
__device__ __forceinline__ void stage_transposed(float* __restrict__ tr, const float* __restrict__ cm, int H, const Rect& t) {
    const int PT = t.th | 1, items = t.vr * t.vc, nt = blockDim.x;
    Walk k(t.vr);                          // q = column, r = row
    for (int i = threadIdx.x; i < items; i += 4 * nt) {
        float v[4];
        int off[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = 0.0f;
            off[u] = -1;
            if (i + u * nt < items) {
                off[u] = k.q * PT + k.r;
                v[u] = cm[(long)(t.w0 + k.q) * H + t.h0 + k.r];
            }
            k.step();
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (off[u] >= 0) tr[off[u]] = v[u];
    }
}

// a[dy][0..5] = image pixels (hl + dy - 1, 4 j - 1 .. 4 j + 4) of the rect: the taps of the run's four pixels
__device__ __forceinline__ void load_window(const float* __restrict__ img, int P, int hl, int j, float (&a)[3][6]) {
    const float* __restrict__ p = img + hl * P + 4 * j + 3;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const float4 v = *reinterpret_cast<const float4*>(p + dy * P + 1);
        a[dy][0] = p[dy * P];
        a[dy][1] = v.x; a[dy][2] = v.y; a[dy][3] = v.z; a[dy][4] = v.w;
        a[dy][5] = p[dy * P + 5];
    }
}

// the first nv pixels of a run
__device__ __forceinline__ void store_run(float* __restrict__ o, int nv, const float (&y)[4], bool vec) {
    if (vec) {
        *reinterpret_cast<float4*>(o) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
        o[0] = y[0];
        if (nv > 1) o[1] = y[1];
        if (nv > 2) o[2] = y[2];
        if (nv > 3) o[3] = y[3];
    }
}

__device__ __forceinline__ float4 load_run(const float* __restrict__ s, int nv, bool vec) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (vec) {
        v = *reinterpret_cast<const float4*>(s);
    } else {
        v.x = s[0];
        if (nv > 1) v.y = s[1];
        if (nv > 2) v.z = s[2];
        if (nv > 3) v.w = s[3];
    }
    return v;
}

__global__ void __launch_bounds__(256) dwconv_silu_fwd_kernel(const DwArgs a) {
    const int H = a.H, W = a.W;
    const long L = (long)H * W;
    const int spp = a.spp, nt = blockDim.x;
    const int lbk = xcd_logical_block((int)blockIdx.x, (int)gridDim.x);   // strips of a plane share lines: same XCD (L2)
    const int plane_id = lbk / spp;                  // b * d + c
    const Rect t = strip_rect(a, lbk - plane_id * spp);
    const int c = plane_id % a.d, b = plane_id / a.d;
    const bool vec = a.vec != 0;
    const float* __restrict__ plane = a.x + x_plane_offset(a, plane_id);
    float* __restrict__ o_rm = a.out2 + ((long)(b * a.orders + 0) * a.d + c) * L;
    float* __restrict__ o_cm = a.out2 + ((long)(b * a.orders + 1) * a.d + c) * L;
    float* __restrict__ sIn = dw_smem;
    float* __restrict__ sT = dw_smem + img_floats(t);
    const int P = t.tw + 8, PT = t.th | 1, RW = (t.vc + 3) >> 2, nruns = t.vr * RW;
    float wk[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) wk[i] = a.w[c * 9 + i];
    const float bias = a.bias ? a.bias[c] : 0.0f;
    stage_image(sIn, plane, H, W, t, vec);
    __syncthreads();
    Walk k(RW);                            // q = row of the rect, r = run of the row
    for (int i = threadIdx.x; i < nruns; i += nt) {
        const int hl = k.q, j = k.r;
        float win[3][6], y[4];
        load_window(sIn, P, hl, j, win);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float acc = bias;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) acc = fmaf(wk[dy * 3 + dx], win[dy][e + dx], acc);
            y[e] = acc * sigmoidf_fast(acc);
        }
        store_run(o_rm + (long)(t.h0 + hl) * W + t.w0 + 4 * j, t.vc - 4 * j, y, vec);
        if (a.orders > 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sT[(4 * j + e) * PT + hl] = y[e];
        }
        k.step();
    }
    if (a.orders < 2) return;
    __syncthreads();
    const int items = t.vr * t.vc;
    Walk q(t.vr);                          // q = column, r = row: stores contiguous along h
    for (int i = threadIdx.x; i < items; i += nt) {
        o_cm[(long)(t.w0 + q.q) * H + t.h0 + q.r] = sT[q.q * PT + q.r];
        q.step();
    }
}

// backward of one rect.  FUSED (whole plane): gpre goes into a bordered LDS image, over the transposed gradient tile it
// was computed from, and dx is the second stencil on that image.  Otherwise gpre is stored and dwconv_bwd2_kernel follows.
// The row-major gradient of a thread's runs is requested first and stays in registers (G) across the staging; the sums
// of a run are a two-level tree, a thread adds its <= MAXR run sums in order, the four waves add pairwise.
template <bool DET, bool FUSED, int MAXR>
__device__ __forceinline__ void dwconv_silu_bwd_rect(const DwArgs& a, const Rect& t, int plane_id, int slot) {
    const int H = a.H, W = a.W;
    const long L = (long)H * W;
    const int c = plane_id % a.d, b = plane_id / a.d;
    const bool vec = a.vec != 0;
    const int tid = threadIdx.x, nt = blockDim.x;
    const float* __restrict__ plane = a.x + x_plane_offset(a, plane_id);
    const float* __restrict__ g_rm = a.g2 + ((long)(b * a.orders + 0) * a.d + c) * L;
    const float* __restrict__ g_cm = a.g2 + ((long)(b * a.orders + 1) * a.d + c) * L;
    float* __restrict__ sIn = dw_smem;                      // x, bordered
    float* __restrict__ sG = dw_smem + img_floats(t);       // transposed column-major gradient, then (FUSED) gpre, bordered
    float* __restrict__ red = sG + (FUSED ? max(img_floats(t), tr_floats(t)) : tr_floats(t));
    const int P = t.tw + 8, PT = t.th | 1, RW = (t.vc + 3) >> 2, nruns = t.vr * RW;
    float wk[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) wk[i] = a.w[c * 9 + i];
    const float bias = a.bias ? a.bias[c] : 0.0f;
    const Walk k0(RW);                     // q = row of the rect, r = run of the row
    float4 G[MAXR];
    {
        Walk k = k0;
#pragma unroll
        for (int r = 0; r < MAXR; ++r) {
            G[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (tid + r * nt < nruns) G[r] = load_run(g_rm + (long)(t.h0 + k.q) * W + t.w0 + 4 * k.r, t.vc - 4 * k.r, vec);
            k.step();
        }
    }
    stage_image(sIn, plane, H, W, t, vec);
    if (a.orders > 1) stage_transposed(sG, g_cm, H, t);
    __syncthreads();
    float acc_w[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    float acc_b = 0.0f;
    {
        Walk k = k0;
#pragma unroll
        for (int r = 0; r < MAXR; ++r) {
            if (tid + r * nt < nruns) {
                const int hl = k.q, j = k.r, nv = t.vc - 4 * j;
                float win[3][6];
                load_window(sIn, P, hl, j, win);
                float g[4] = {G[r].x, G[r].y, G[r].z, G[r].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pre = bias;
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) pre = fmaf(wk[dy * 3 + dx], win[dy][e + dx], pre);
                    const float sg = sigmoidf_fast(pre);
                    const float dsilu = sg * fmaf(pre, 1.0f - sg, 1.0f);           // d/dp [p * sigmoid(p)]
                    const float gc = a.orders > 1 ? sG[(4 * j + e) * PT + hl] : 0.0f;
                    const float v = (g[e] + gc) * dsilu;
                    g[e] = e < nv ? v : 0.0f;          // pixels past the plane's edge: no sum, and the zero border of gpre
                }
                const float sb = (g[0] + g[1]) + (g[2] + g[3]);
                acc_b = r == 0 ? sb : acc_b + sb;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const float s = fmaf(g[1], win[dy][1 + dx], g[0] * win[dy][dx]) + fmaf(g[3], win[dy][3 + dx], g[2] * win[dy][2 + dx]);
                        acc_w[dy * 3 + dx] = r == 0 ? s : acc_w[dy * 3 + dx] + s;
                    }
                if constexpr (FUSED) G[r] = make_float4(g[0], g[1], g[2], g[3]);
                else store_run(a.gpre + (long)plane_id * L + (long)(t.h0 + hl) * W + t.w0 + 4 * j, nv, g, vec);
            }
            k.step();
        }
    }
    if constexpr (FUSED) {
        float* __restrict__ dx = a.dx + x_plane_offset(a, plane_id);
        __syncthreads();                   // every thread has read its column-major gradient out of sG
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const int G4 = (t.tw >> 2) + 2;
        for (int i = tid; i < 2 * G4 + 2 * t.th; i += nt) {          // top and bottom rows, first and last group of a row
            int row, grp;
            if (i < 2 * G4) { row = i < G4 ? 0 : t.th + 1; grp = i < G4 ? i : i - G4; }
            else { const int e = i - 2 * G4; row = 1 + (e >> 1); grp = (e & 1) ? G4 - 1 : 0; }
            *reinterpret_cast<float4*>(sG + row * P + 4 * grp) = zero;
        }
        {
            Walk k = k0;
#pragma unroll
            for (int r = 0; r < MAXR; ++r) {
                if (tid + r * nt < nruns) *reinterpret_cast<float4*>(sG + (k.q + 1) * P + 4 + 4 * k.r) = G[r];
                k.step();
            }
        }
        __syncthreads();
        {
            Walk k = k0;
#pragma unroll
            for (int r = 0; r < MAXR; ++r) {
                if (tid + r * nt < nruns) {
                    const int hl = k.q, j = k.r;
                    float win[3][6], y[4];
                    load_window(sG, P, hl, j, win);    // win[dy][e + dx] = gpre[h + dy - 1][w + dx - 1] of pixel e
                    // y[h'][w'] used x[h][w] with tap (h - h' + 1, w - w' + 1): dx[h][w] = sum_k W[8-k] * gpre tap k
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float acc = 0.0f;
#pragma unroll
                        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                            for (int dx_ = 0; dx_ < 3; ++dx_) acc = fmaf(wk[8 - (dy * 3 + dx_)], win[dy][e + dx_], acc);
                        y[e] = acc;
                    }
                    store_run(dx + (long)(t.h0 + hl) * W + t.w0 + 4 * j, t.vc - 4 * j, y, vec);
                }
                k.step();
            }
        }
    }
    // block reduction of the 10 per-channel sums, then one atomic (or slot store) each
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float s = wave_sum_shfl(acc_w[k]);
        if (lane == 0) red[wave * 10 + k] = s;
    }
    {
        const float s = wave_sum_shfl(acc_b);
        if (lane == 0) red[wave * 10 + 9] = s;
    }
    if (tid >= (nt >> 6) * 10 && tid < 40) red[tid] = 0.0f;        // waves the workgroup does not have
    __syncthreads();
    if (tid < 10) dw_leave<DET>(a, c, slot, tid, (red[tid] + red[10 + tid]) + (red[20 + tid] + red[30 + tid]));
}

template <bool DET>
__device__ __forceinline__ void dwconv_silu_bwd1_body(const DwArgs& a) {
    const int spp = a.spp;
    const int lbk = xcd_logical_block((int)blockIdx.x, (int)gridDim.x);
    const int plane_id = lbk / spp, strip_id = lbk - plane_id * spp;
    dwconv_silu_bwd_rect<DET, false, kStripRuns>(a, strip_rect(a, strip_id), plane_id, (plane_id / a.d) * spp + strip_id);
}

__global__ void __launch_bounds__(256) dwconv_silu_bwd1_kernel(const DwArgs a) { dwconv_silu_bwd1_body<false>(a); }
// deterministic mode (SIGMA_DWCONV_DETERMINISTIC): the sums go to a.part, dwconv_reduce_kernel adds them
__global__ void __launch_bounds__(256) dwconv_silu_bwd1_det_kernel(const DwArgs a) { dwconv_silu_bwd1_body<true>(a); }

__global__ void __launch_bounds__(256) dwconv_bwd2_kernel(const DwArgs a) {
    const int H = a.H, W = a.W;
    const long L = (long)H * W;
    const int spp = a.spp, nt = blockDim.x;
    const int lbk = xcd_logical_block((int)blockIdx.x, (int)gridDim.x);
    const int plane_id = lbk / spp;
    const Rect t = strip_rect(a, lbk - plane_id * spp);
    const int c = plane_id % a.d;
    const bool vec = a.vec != 0;
    float* __restrict__ dx = a.dx + x_plane_offset(a, plane_id);
    float* __restrict__ sG = dw_smem;
    const int P = t.tw + 8, RW = (t.vc + 3) >> 2, nruns = t.vr * RW;
    float wk[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) wk[i] = a.w[c * 9 + i];
    stage_image(sG, a.gpre + (long)plane_id * L, H, W, t, vec);
    __syncthreads();
    Walk k(RW);
    for (int i = threadIdx.x; i < nruns; i += nt) {
        const int hl = k.q, j = k.r;
        float win[3][6], y[4];
        load_window(sG, P, hl, j, win);        // win[dy][e + dx] = gpre[h + dy - 1][w + dx - 1] of pixel e
        // y[h'][w'] used x[h][w] with tap (h - h' + 1, w - w' + 1): dx[h][w] = sum_k W[8-k] * gpre tap k
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float acc = 0.0f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx_ = 0; dx_ < 3; ++dx_) acc = fmaf(wk[8 - (dy * 3 + dx_)], win[dy][e + dx_], acc);
            y[e] = acc;
        }
        store_run(dx + (long)(t.h0 + hl) * W + t.w0 + 4 * j, t.vc - 4 * j, y, vec);
        k.step();
    }
}

// ---- whole-plane backward --------------------------------------------------------------------------------------------
// Planes below the 48 KiB line of the gpre contract (everything below the 120 x 160 first stage): ONE workgroup owns a
// whole (batch, channel) plane and keeps the pre-activation gradient in LDS between its two stencils (no gpre round trip
// through HBM, one launch instead of two).
//
// Compact body: a plane of one or a few columns and a thousand rows is below the line with its (W + 2) | 1 pitch but not
// with the bordered image's W + 8.  It keeps the one-pixel border, scalar taps and a pixel per thread and step.
__device__ __forceinline__ int plane_pitch(int W) { return (W + 2) | 1; }

template <bool DET>
__device__ __forceinline__ void dwconv_silu_bwd_plane_compact_body(const DwArgs& a) {
    const int H = a.H, W = a.W, L = H * W, pitch = plane_pitch(W);
    float* __restrict__ sIn = dw_smem;                       // x, zero border
    float* __restrict__ sG = dw_smem + (H + 2) * pitch;      // column-major gradient, then gpre; zero border
    float* __restrict__ red = dw_smem + 2 * (H + 2) * pitch;
    const int plane_id = blockIdx.x;
    const int c = plane_id % a.d, b = plane_id / a.d;
    const int tid = threadIdx.x;
    const float* __restrict__ plane = a.x + x_plane_offset(a, plane_id);
    const float* __restrict__ g_rm = a.g2 + ((long)(b * a.orders + 0) * a.d + c) * L;
    const float* __restrict__ g_cm = a.g2 + ((long)(b * a.orders + 1) * a.d + c) * L;
    float* __restrict__ dx = a.dx + x_plane_offset(a, plane_id);
    for (int i = tid; i < 2 * (H + 2) * pitch; i += 256) dw_smem[i] = 0.0f;
    __syncthreads();
    for (int idx = tid; idx < L; idx += 256) { const int h = idx / W, w = idx - h * W; sIn[(h + 1) * pitch + (w + 1)] = plane[idx]; }
    if (a.orders > 1)
        for (int idx = tid; idx < L; idx += 256) { const int w = idx / H, h = idx - w * H; sG[(h + 1) * pitch + (w + 1)] = g_cm[idx]; }
    __syncthreads();
    float wk[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) wk[i] = a.w[c * 9 + i];
    const float bias = a.bias ? a.bias[c] : 0.0f;
    float acc_w[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    float acc_b = 0.0f;
    for (int idx = tid; idx < L; idx += 256) {
        const int h = idx / W, w = idx - h * W;
        const float* __restrict__ p = sIn + h * pitch + w;
        float t[9];
        float pre = bias;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx_ = 0; dx_ < 3; ++dx_) { t[dy * 3 + dx_] = p[dy * pitch + dx_]; pre = fmaf(wk[dy * 3 + dx_], t[dy * 3 + dx_], pre); }
        const float sg = sigmoidf_fast(pre);
        const float dsilu = sg * fmaf(pre, 1.0f - sg, 1.0f);
        float* __restrict__ own = sG + (h + 1) * pitch + (w + 1);       // read and written by this thread only
        const float g = (g_rm[idx] + *own) * dsilu;
        *own = g;
        acc_b += g;
#pragma unroll
        for (int k = 0; k < 9; ++k) acc_w[k] = fmaf(g, t[k], acc_w[k]);
    }
    __syncthreads();
    for (int idx = tid; idx < L; idx += 256) {
        const int h = idx / W, w = idx - h * W;
        const float* __restrict__ q = sG + h * pitch + w;              // gpre[h - 1][w - 1]
        float acc = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx_ = 0; dx_ < 3; ++dx_) acc = fmaf(wk[8 - (dy * 3 + dx_)], q[dy * pitch + dx_], acc);
        dx[idx] = acc;
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float s = wave_sum_shfl(acc_w[k]);
        if (lane == 0) red[wave * 10 + k] = s;
    }
    {
        const float s = wave_sum_shfl(acc_b);
        if (lane == 0) red[wave * 10 + 9] = s;
    }
    __syncthreads();
    if (tid < 10) dw_leave<DET>(a, c, b, tid, red[tid] + red[10 + tid] + red[20 + tid] + red[30 + tid]);
}

template <bool DET>
__device__ __forceinline__ void dwconv_silu_bwd_plane_body(const DwArgs& a) {
    if (a.compact) { dwconv_silu_bwd_plane_compact_body<DET>(a); return; }
    const int plane_id = blockIdx.x;
    const int tw = (a.W + 3) & ~3;
    dwconv_silu_bwd_rect<DET, true, kPlaneRuns>(a, Rect{0, 0, a.H, tw, a.H, a.W}, plane_id, plane_id / a.d);
}

__global__ void __launch_bounds__(256) dwconv_silu_bwd_plane_kernel(const DwArgs a) { dwconv_silu_bwd_plane_body<false>(a); }
__global__ void __launch_bounds__(256) dwconv_silu_bwd_plane_det_kernel(const DwArgs a) { dwconv_silu_bwd_plane_body<true>(a); }

// deterministic mode: dweight / dbias = the sums of the `slots` workgroup slots of a.part, slot 0 first (fixed order)
__global__ void __launch_bounds__(256) dwconv_reduce_kernel(const DwArgs a, int slots) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < a.d * 10; e += gridDim.x * blockDim.x) {
        const int c = e / 10, k = e - c * 10;
        if (k == 9 && !a.dbias) continue;
        float acc = 0.0f;
        for (int sl = 0; sl < slots; ++sl) acc += a.part[(long)sl * a.d * 10 + e];
        if (k < 9) a.dw[c * 9 + k] = acc;
        else a.dbias[c] = acc;
    }
}

// the 48 KiB line of the gpre contract (sigma_ops.h): two (H + 2) x ((W + 2) | 1) images; below it the backward is one
// whole-plane launch and p->gpre is not touched
bool plane_below_line(const sigma_dwconv_params* p) {
    const long pitch = (p->width + 2) | 1;
    return 2L * (p->height + 2) * pitch * (long)sizeof(float) <= 48 * 1024;
}

constexpr long kRedFloats = 40;            // the 4 x 10 wave sums of a backward workgroup

// LDS bytes of the whole-plane backward on the bordered image, 0 = the plane takes the compact body
size_t plane_rect_lds_bytes(const sigma_dwconv_params* p) {
    const long tw = (p->width + 3) & ~3L, H = p->height;
    const long img = (H + 2) * (tw + 8), tr = (tw * (H | 1) + 3) & ~3L;
    const long bytes = (img + (img > tr ? img : tr) + kRedFloats) * (long)sizeof(float);
    const bool runs_fit = H * (tw >> 2) <= (long)kPlaneRuns * kThreads;      // threads_for: 256 threads above 768 runs
    return runs_fit && bytes <= 64 * 1024 ? (size_t)bytes : 0;
}

size_t plane_compact_lds_bytes(const sigma_dwconv_params* p) {
    const long pitch = (p->width + 2) | 1;
    return (size_t)((2L * (p->height + 2) * pitch + kRedFloats) * (long)sizeof(float));
}

int check(const sigma_dwconv_params* p) {
    if (!p) return fail(SIGMA_OPS_ERR_ARG, "params is NULL");
    if (p->flags & ~SIGMA_DWCONV_DETERMINISTIC) return fail(SIGMA_OPS_ERR_ARG, "unknown bits in flags (0x%x)", (unsigned)p->flags);
    if (p->batch < 0 || p->channels <= 0 || p->height <= 0 || p->width <= 0)
        return fail(SIGMA_OPS_ERR_ARG, "bad sizes batch=%d channels=%d height=%d width=%d", p->batch, p->channels, p->height, p->width);
    if (p->n_orders != 1 && p->n_orders != 2) return fail(SIGMA_OPS_ERR_ARG, "n_orders must be 1 or 2 (got %d)", p->n_orders);
    const long tiles = (long)((p->width + kTile - 1) / kTile) * ((p->height + kTile - 1) / kTile);
    if ((long)p->batch * p->channels * tiles > 2147483647L)
        return fail(SIGMA_OPS_ERR_ARG, "batch %d x channels %d x %ld tiles exceed the grid limit of 2^31 - 1", p->batch, p->channels, tiles);
    return SIGMA_OPS_OK;
}

// strips of a plane: ceil(H / 32) rows of strips of equal height, each cut into as few pieces of <= 4 x 32 columns as
// cover the width, of equal width in 32-column tiles.  Never more workgroups than the 32 x 32 tiles of the plane.
struct Strips { int th, rows, m, nblk; };

Strips strips_for(const sigma_dwconv_params* p) {
    Strips s;
    s.rows = (p->height + kTile - 1) / kTile;
    s.th = (p->height + s.rows - 1) / s.rows;
    const int tw_n = (p->width + kTile - 1) / kTile;
    s.nblk = (tw_n + kStripTiles - 1) / kStripTiles;
    s.m = (tw_n + s.nblk - 1) / s.nblk;
    return s;
}

void set_strips(const sigma_dwconv_params* p, DwArgs& a) {
    const Strips s = strips_for(p);
    a.th = s.th; a.m = s.m; a.nblk = s.nblk; a.spp = s.rows * s.nblk;
}

// threads of a workgroup whose rect has `runs` runs of four pixels: about three runs per thread, whole waves.  A 15 x 20
// plane (75 runs) takes one wave, 30 x 40 two: what a wave spends outside its runs (indices, weights, barriers) is paid
// per wave, and more workgroups fit a CU.
unsigned threads_for(long runs) {
    const long t = ((runs + 2) / 3 + 63) / 64 * 64;
    return (unsigned)(t < 64 ? 64 : t > kThreads ? kThreads : t);
}

unsigned strip_threads(const sigma_dwconv_params* p) {
    const Strips s = strips_for(p);
    const long w = p->width < kTile * s.m ? p->width : kTile * s.m;
    return threads_for((long)s.th * ((w + 3) / 4));
}

dim3 grid_for(const sigma_dwconv_params* p) {
    const Strips s = strips_for(p);
    return dim3((unsigned)((long)s.rows * s.nblk * p->batch * p->channels));
}

// LDS bytes of a strip workgroup: the bordered image, the transposed tile (forward, bwd1), the wave sums (bwd1)
size_t strip_lds_bytes(const sigma_dwconv_params* p, bool transposed, bool sums) {
    const Strips s = strips_for(p);
    const long tw = (long)kTile * s.m;
    long fl = (s.th + 2) * (tw + 8);
    if (transposed) fl += (tw * (s.th | 1) + 3) & ~3L;
    if (sums) fl += kRedFloats;
    return (size_t)(fl * (long)sizeof(float));
}

// workgroup slots the deterministic workspace is sized for: one per (batch, 32 x 32 tile) and channel (whole plane: one tile)
long det_slots(const sigma_dwconv_params* p) {
    const long tiles = plane_below_line(p) ? 1 : (long)((p->width + kTile - 1) / kTile) * ((p->height + kTile - 1) / kTile);
    return tiles * p->batch;
}

// slots the backward writes and dwconv_reduce_kernel reads: one per (batch, strip) -- never more than det_slots
long det_slots_used(const sigma_dwconv_params* p) {
    if (plane_below_line(p)) return p->batch;
    const Strips s = strips_for(p);
    return (long)s.rows * s.nblk * p->batch;
}

}  // namespace

}  // namespace sigma

namespace sigma {
// plane strides of x / dx: 0 / 0 = packed (B, d, H, W); otherwise both given, planes contiguous and non-overlapping
int plane_strides(const sigma_dwconv_params* p, DwArgs& a) {
    const long L = (long)p->height * p->width;
    if (p->x_batch_stride == 0 && p->x_channel_stride == 0) { a.x_bs = (long)p->channels * L; a.x_cs = L; return SIGMA_OPS_OK; }
    if (p->x_batch_stride < L || p->x_channel_stride < L)
        return fail(SIGMA_OPS_ERR_ARG, "x_batch_stride %lld and x_channel_stride %lld must both be 0 or at least one plane (%ld)",
                    (long long)p->x_batch_stride, (long long)p->x_channel_stride, L);
    a.x_bs = p->x_batch_stride; a.x_cs = p->x_channel_stride;
    return SIGMA_OPS_OK;
}
}  // namespace sigma

extern "C" {

int sigma_dwconv3x3_silu_fwd(const sigma_dwconv_params* p, void* stream) {
    int rc = sigma::check(p);
    if (rc) return rc;
    if (p->batch == 0) return SIGMA_OPS_OK;
    if (!p->x || !p->weight || !p->out2) return sigma::fail(SIGMA_OPS_ERR_ARG, "x, weight and out2 must be non-NULL device pointers");
    sigma::DwArgs a{};
    a.x = p->x; a.w = p->weight; a.bias = p->bias; a.out2 = p->out2;
    a.B = p->batch; a.d = p->channels; a.H = p->height; a.W = p->width; a.orders = p->n_orders;
    if ((rc = sigma::plane_strides(p, a))) return rc;
    sigma::set_strips(p, a);
    // 16-byte accesses: every row of every plane starts on a 16-byte boundary (W % 4 == 0 makes L % 4 == 0)
    a.vec = (p->width & 3) == 0 && (a.x_bs & 3) == 0 && (a.x_cs & 3) == 0 && sigma::aligned(p->x, 16) && sigma::aligned(p->out2, 16);
    hipLaunchKernelGGL(sigma::dwconv_silu_fwd_kernel, sigma::grid_for(p), dim3(sigma::strip_threads(p)), sigma::strip_lds_bytes(p, true, false),
                       static_cast<hipStream_t>(stream), a);
    return sigma::launched("dwconv_silu_fwd_kernel");
}

int64_t sigma_dwconv3x3_silu_bwd_workspace_bytes(const sigma_dwconv_params* p) {
    if (sigma::check(p)) return -1;
    if (!(p->flags & SIGMA_DWCONV_DETERMINISTIC)) return 0;
    return (int64_t)sigma::det_slots(p) * p->channels * 10 * (int64_t)sizeof(float);
}

int sigma_dwconv3x3_silu_bwd(const sigma_dwconv_params* p, void* stream) {
    int rc = sigma::check(p);
    if (rc) return rc;
    if (p->batch == 0) {
        // deterministic mode: dweight / dbias are written -- with no batch, as zeros
        if (!(p->flags & SIGMA_DWCONV_DETERMINISTIC)) return SIGMA_OPS_OK;
        if (!p->dweight) return sigma::fail(SIGMA_OPS_ERR_ARG, "dweight is NULL (deterministic mode writes it for an empty batch too)");
        hipStream_t s = static_cast<hipStream_t>(stream);
        hipError_t e = hipMemsetAsync(p->dweight, 0, (size_t)p->channels * 9 * sizeof(float), s);
        if (e == hipSuccess && p->dbias) e = hipMemsetAsync(p->dbias, 0, (size_t)p->channels * sizeof(float), s);
        return sigma::launched("hipMemsetAsync of dweight / dbias", e);
    }
    if (!p->x || !p->weight || !p->g2 || !p->gpre || !p->dweight || !p->dx)
        return sigma::fail(SIGMA_OPS_ERR_ARG, "x, weight, g2, gpre, dweight and dx must be non-NULL device pointers");
    const bool det = (p->flags & SIGMA_DWCONV_DETERMINISTIC) != 0;
    const int64_t need = sigma_dwconv3x3_silu_bwd_workspace_bytes(p);
    if (det && (!p->workspace || p->workspace_bytes < need || !sigma::aligned(p->workspace, 16)))
        return sigma::fail(SIGMA_OPS_ERR_ARG, "deterministic mode needs a 16-byte aligned workspace of %lld bytes (got %p, %lld bytes)",
                           (long long)need, p->workspace, (long long)p->workspace_bytes);
    sigma::DwArgs a{};
    a.x = p->x; a.w = p->weight; a.bias = p->bias; a.g2 = p->g2; a.gpre = p->gpre;
    a.dw = p->dweight; a.dbias = p->dbias; a.dx = p->dx;
    a.B = p->batch; a.d = p->channels; a.H = p->height; a.W = p->width; a.orders = p->n_orders;
    a.part = det ? static_cast<float*>(p->workspace) : nullptr;
    if ((rc = sigma::plane_strides(p, a))) return rc;
    sigma::set_strips(p, a);
    const bool plane = sigma::plane_below_line(p);
    a.vec = (p->width & 3) == 0 && (a.x_bs & 3) == 0 && (a.x_cs & 3) == 0 && sigma::aligned(p->x, 16) && sigma::aligned(p->dx, 16) &&
            sigma::aligned(p->g2, 16) && (plane || sigma::aligned(p->gpre, 16));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (plane) {                                             // one launch, gpre stays in LDS (p->gpre is not written)
        size_t lds = sigma::plane_rect_lds_bytes(p);
        a.compact = lds == 0;
        if (a.compact) lds = sigma::plane_compact_lds_bytes(p);
        hipLaunchKernelGGL(det ? sigma::dwconv_silu_bwd_plane_det_kernel : sigma::dwconv_silu_bwd_plane_kernel,
                           dim3((unsigned)(p->batch * p->channels)),
                           dim3(a.compact ? 256u : sigma::threads_for((long)p->height * ((p->width + 3) / 4))), lds, s, a);
        if ((rc = sigma::launched(det ? "dwconv_silu_bwd_plane_det_kernel" : "dwconv_silu_bwd_plane_kernel"))) return rc;
    } else {
        hipLaunchKernelGGL(det ? sigma::dwconv_silu_bwd1_det_kernel : sigma::dwconv_silu_bwd1_kernel, sigma::grid_for(p),
                           dim3(sigma::strip_threads(p)), sigma::strip_lds_bytes(p, true, true), s, a);
        if ((rc = sigma::launched(det ? "dwconv_silu_bwd1_det_kernel" : "dwconv_silu_bwd1_kernel"))) return rc;
        hipLaunchKernelGGL(sigma::dwconv_bwd2_kernel, sigma::grid_for(p), dim3(sigma::strip_threads(p)), sigma::strip_lds_bytes(p, false, false), s, a);
        if ((rc = sigma::launched("dwconv_bwd2_kernel"))) return rc;
    }
    if (det) {
        const int blocks = (p->channels * 10 + 255) / 256;
        hipLaunchKernelGGL(sigma::dwconv_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, (int)sigma::det_slots_used(p));
        if ((rc = sigma::launched("dwconv_reduce_kernel"))) return rc;
    }
    return SIGMA_OPS_OK;
}

}  // extern "C"
