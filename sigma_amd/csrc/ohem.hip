// ohem.hip -- online hard example mining for the segmentation loss: which pixels the cross entropy keeps, chosen on the device.
//
// Reference: ProbOhemCrossEntropy2d (utils/loss_opr.py:137-187): the probability of the labelled class p, 1 at ignored
// pixels; the min_kept-th smallest p, raised to `thresh` where it is below it, is the threshold; pixels with p above it
// are given the ignore label and nn.CrossEntropyLoss runs on the rest.  Here the same selection on nll = lse - x_y =
// -log p, which sigma_softmax_ce_opt_fwd writes as its row loss (weight NULL, eps 0): p <= t  <=>  nll >= -log t, so the
// k-th LARGEST nll is looked for, tau = min(-log thresh, that value), and a labelled row is kept unless nll < tau.
//
//   ohem_init    zero fill of the workspace
//   ohem_hist    one digit (8 bits, most significant first) of the order-preserving unsigned image of the keys: every
//                workgroup counts the labelled rows whose higher digits equal the prefix found so far into an LDS
//                histogram, then adds its non-empty bins to the pass's global histogram (one integer atomic per bin)
//   ohem_pick    one workgroup: walks the 256 bins from the top until the rank is reached, appends the digit to the
//                prefix and keeps the rank inside the bin.  The first pass also yields the number of labelled rows and
//                decides whether anything is mined at all (min_kept in [1, num_valid]); the last one hands
//                counts[0] = num_valid, counts[1] = 0 to the final kernel
//   ohem_final   tau from the full prefix; mined[r] = label or ignore_index; optionally the weighted row losses and the
//                SIGMA_CE_BLOCKS partial (loss, weight) pairs of the cross entropy ON the mined labels, in the row -> thread
//                order and with the block_sum of softmax_ce_fwd_*kernel (pointwise.hip), so that the bits are those a second
//                forward over the logits would give; the kept rows are counted with one integer atomic per workgroup
//
// Four counting passes over 4-byte keys and 8-byte labels and one final pass; the logits are not read.  Only integer atomics:
// the result does not depend on the order of arrival.  Every launch is unconditional and nothing is read back: whether
// rows are mined is a flag in the workspace, so a captured graph replays whatever the data say.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ops_host.h"
#include "scan_device.h"

namespace sigma {
namespace {

constexpr int kOhemBins = 256;           // 8-bit digits
constexpr int kOhemPasses = 4;
constexpr int kOhemHistBlocks = SIGMA_OHEM_HIST_BLOCKS;

// the workspace: kOhemPasses histograms of kOhemBins counters (zero-filled by ohem_init_kernel), then this
struct OhemState {
    uint32_t prefix;       // the digits found so far, in place
    uint32_t rank;         // 1-based rank from the top among the rows that share the prefix
    uint32_t num_valid;
    uint32_t mine;         // 0: every labelled row is kept (rule 1)
};

// ascending unsigned order == ascending float order (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN)
__device__ __forceinline__ uint32_t ohem_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float ohem_unkey(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

__device__ __forceinline__ bool ohem_valid(long y, long ignore, int nc) { return y != ignore && y >= 0 && y < nc; }

// zero fill of the histograms and the state.  A kernel, not a memset: as a memset node of a captured graph the fill did
// not reach the replay (the histograms kept the counts of earlier runs and the replay mined where eager did not)
__global__ void __launch_bounds__(256) ohem_init_kernel(uint32_t* __restrict__ ws, int words) {
    for (int i = threadIdx.x; i < words; i += blockDim.x) ws[i] = 0u;
}

__global__ void __launch_bounds__(256)
ohem_hist_kernel(const float* __restrict__ nll, const int64_t* __restrict__ labels, long rows, int nc, long ignore, int pass,
                 const OhemState* __restrict__ st, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kOhemBins];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t high = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);       // the digits already fixed
    const uint32_t prefix = pass == 0 ? 0u : st->prefix;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        if (!ohem_valid(labels[r], ignore, nc)) continue;
        const uint32_t k = ohem_key(nll[r]);
        if (((k ^ prefix) & high) == 0u) atomicAdd(&h[(k >> shift) & (kOhemBins - 1)], 1u);
    }
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
}

__global__ void __launch_bounds__(256)
ohem_pick_kernel(const uint32_t* __restrict__ hist, OhemState* __restrict__ st, int pass, long min_kept, int64_t* __restrict__ counts) {
    __shared__ uint32_t h[kOhemBins];
    h[threadIdx.x] = hist[threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t rank, prefix;
    if (pass == 0) {
        uint32_t nv = 0u;                                   // rows <= 2^31 - 1
        for (int b = 0; b < kOhemBins; ++b) nv += h[b];
        const bool mine = min_kept > 0 && nv > 0u && (uint64_t)min_kept <= (uint64_t)nv;
        st->num_valid = nv;
        st->mine = mine ? 1u : 0u;
        rank = mine ? (uint32_t)min_kept : 1u;
        prefix = 0u;
    } else {
        rank = st->rank;
        prefix = st->prefix;
    }
    uint32_t above = 0u;
    int digit = 0;
    bool found = false;
    for (int b = kOhemBins - 1; b >= 0; --b) {
        if (above + h[b] >= rank) { digit = b; found = true; break; }
        above += h[b];
    }
    st->rank = found ? rank - above : 1u;                   // not found: no labelled row at all; nothing is mined then
    st->prefix = prefix | ((uint32_t)digit << (24 - 8 * pass));
    if (pass == kOhemPasses - 1) { counts[0] = (int64_t)st->num_valid; counts[1] = 0; }
}

__global__ void __launch_bounds__(256)
ohem_final_kernel(const float* __restrict__ nll, const int64_t* __restrict__ labels, const float* __restrict__ w, long rows, int nc,
                  long ignore, float nl_thresh, const OhemState* __restrict__ st, int64_t* __restrict__ mined,
                  float* __restrict__ tau_out, int64_t* __restrict__ counts, float* __restrict__ row_loss, float* __restrict__ partial) {
    __shared__ float sh[4];
    __shared__ uint32_t kept_sh[4];
    const float kth = ohem_unkey(st->prefix);
    const float tau = st->mine ? (kth < nl_thresh ? kth : nl_thresh) : -INFINITY;
    if (blockIdx.x == 0 && threadIdx.x == 0) tau_out[0] = tau;
    float loss = 0.0f, den = 0.0f;
    uint32_t kept = 0u;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const long y = labels[r];
        const float v = nll[r];
        const bool keep = ohem_valid(y, ignore, nc) && !(v < tau);       // a NaN key is kept: the loss is NaN, as without mining
        mined[r] = keep ? y : ignore;
        float rl = 0.0f;
        if (keep) {
            const float wy = w ? w[y] : 1.0f;
            rl = ((1.0f - 0.0f) * wy) * v;                   // ce_opt_row_loss at eps = 0 on l - x_y = v
            loss += rl;
            den += wy;
            ++kept;
        }
        if (row_loss) row_loss[r] = rl;
    }
    if (partial) {
        const float tl = block_sum(loss, sh);
        const float td = block_sum(den, sh);
        if (threadIdx.x == 0) { partial[2 * blockIdx.x] = tl; partial[2 * blockIdx.x + 1] = td; }
    }
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    if ((threadIdx.x & 63) == 0) kept_sh[threadIdx.x >> 6] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = (kept_sh[0] + kept_sh[1]) + (kept_sh[2] + kept_sh[3]);
        if (t) atomicAdd(reinterpret_cast<unsigned long long*>(counts + 1), (unsigned long long)t);
    }
}

constexpr int64_t kOhemWorkspaceBytes = (int64_t)kOhemPasses * kOhemBins * sizeof(uint32_t) + 64;      // histograms + state, 16-byte sized

}  // namespace
}  // namespace sigma

extern "C" {

int64_t sigma_ohem_workspace_bytes(int64_t rows) {
    if (rows < 0 || rows > 2147483647L) return sigma::fail(-1, "rows %lld must be in [0, 2^31 - 1]", (long long)rows);
    return sigma::kOhemWorkspaceBytes;
}

int sigma_ohem_select(const sigma_ohem_params* p, void* stream) {
    using namespace sigma;
    if (!p) return fail(SIGMA_OPS_ERR_ARG, "params is NULL");
    if (p->rows < 0 || p->rows > 2147483647L || p->classes < 1)
        return fail(SIGMA_OPS_ERR_ARG, "rows %lld must be in [0, 2^31 - 1] and classes %d at least 1", (long long)p->rows, p->classes);
    if (!(p->thresh > 0.0f && p->thresh <= 1.0f)) return fail(SIGMA_OPS_ERR_ARG, "thresh %g must be in (0, 1]", (double)p->thresh);   // NaN fails both
    if (!p->tau || !p->counts || !p->workspace) return fail(SIGMA_OPS_ERR_ARG, "tau, counts and workspace must be non-NULL device pointers");
    if (p->rows > 0 && (!p->nll || !p->labels || !p->mined))
        return fail(SIGMA_OPS_ERR_ARG, "nll, labels and mined must be non-NULL device pointers when rows > 0");
    if (!aligned(p->nll, 4) || !aligned(p->tau, 4) || !aligned(p->weight, 4) || !aligned(p->row_loss, 4) || !aligned(p->partial, 4) ||
        !aligned(p->labels, 8) || !aligned(p->mined, 8) || !aligned(p->counts, 8) || !aligned(p->workspace, 16))
        return fail(SIGMA_OPS_ERR_ARG, "alignment: nll, tau, weight, row_loss and partial need 4 bytes, labels, mined and counts 8, workspace 16");
    if (p->workspace_bytes < kOhemWorkspaceBytes)
        return fail(SIGMA_OPS_ERR_ARG, "workspace of %lld bytes required (got %lld)", (long long)kOhemWorkspaceBytes, (long long)p->workspace_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* hist = static_cast<uint32_t*>(p->workspace);
    OhemState* state = reinterpret_cast<OhemState*>(hist + kOhemPasses * kOhemBins);
    hipLaunchKernelGGL(ohem_init_kernel, dim3(1), dim3(256), 0, st, hist, (int)(kOhemWorkspaceBytes / sizeof(uint32_t)));
    long blocks = ((long)p->rows + 255) / 256;
    blocks = blocks < 1 ? 1 : blocks > kOhemHistBlocks ? kOhemHistBlocks : blocks;
    const float nl_thresh = (float)(0.0 - log((double)p->thresh));
    for (int pass = 0; pass < kOhemPasses; ++pass) {
        hipLaunchKernelGGL(ohem_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p->nll, p->labels, (long)p->rows, (int)p->classes,
                           (long)p->ignore_index, pass, state, hist + pass * kOhemBins);
        hipLaunchKernelGGL(ohem_pick_kernel, dim3(1), dim3(256), 0, st, hist + pass * kOhemBins, state, pass, (long)p->min_kept, p->counts);
    }
    hipLaunchKernelGGL(ohem_final_kernel, dim3(SIGMA_CE_BLOCKS), dim3(256), 0, st, p->nll, p->labels, p->weight, (long)p->rows,
                       (int)p->classes, (long)p->ignore_index, nl_thresh, state, p->mined, p->tau, p->counts, p->row_loss, p->partial);
    return launched("ohem kernels");
}

}  // extern "C"
