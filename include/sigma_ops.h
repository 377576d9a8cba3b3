/*
 * sigma_ops.h -- C ABI of the fused layout / stencil operators around the scan in libsigma_hip.so.
 *
 * These replace torch op sequences of the reference's SS2D block (models/encoders/vmamba.py), they
 * have no counterpart in the reference's native code (which only has the selective-scan kernels):
 *
 *   sigma_dwconv3x3_silu_fwd / _bwd
 *       SS2D.forward, vmamba.py:1071-1072:  x = x.permute(0,3,1,2).contiguous(); x = act(conv2d(x))
 *       with conv2d = nn.Conv2d(d, d, 3, padding=1, groups=d, bias) (vmamba.py:683-691), fused with
 *       the layout half of CrossScan (vmamba.py:80-89): the activation is written once in row-major
 *       and once in column-major sequence order, which is all the scan kernels need (the two
 *       flipped directions are read backwards, see sigma_scan.h rev_group_mask).
 *
 * Same conventions as sigma_scan.h: device pointers, float32, contiguous tensors, the callee
 * enqueues on `stream` (hipStream_t as void*) of the current device, never allocates, never
 * synchronises; returns 0 or a SIGMA_OPS_ERR_* code.
 *
 * The reason of a refusal: every non-zero status, and every *_workspace_bytes query that answers -1,
 * leaves its reason -- what was tested and the offending values, or the kernel and HIP's error for
 * SIGMA_OPS_ERR_LAUNCH -- in the library's thread-local error text, read with sigma_scan_last_error()
 * (sigma_scan.h) on the same thread right after the call.  A success does not touch the text.
 */
#ifndef SIGMA_OPS_H_
#define SIGMA_OPS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum sigma_ops_status {
    SIGMA_OPS_OK = 0,
    SIGMA_OPS_ERR_ARG = 1,
    SIGMA_OPS_ERR_LAUNCH = 5
};

typedef struct sigma_dwconv_params {
    int32_t batch, channels, height, width;
    int32_t n_orders;      /* 2: out2/g2 hold the row-major AND the column-major sequence (SS2D);
                              1: row-major only, i.e. plain conv + SiLU (CroMB / ConMB, vmamba.py:1629-1630,
                              1271-1272) */
    int32_t flags;         /* ABI 11: SIGMA_DWCONV_* bits; 0 = the contract below                   */
    const float *x;        /* (B, d, H, W)   input of the convolution                              */
    const float *weight;   /* (d, 1, 3, 3)                                                         */
    const float *bias;     /* (d) or NULL                                                          */
    /* forward */
    float *out2;           /* (B, n_orders, d, H*W): [:,0] = silu(conv(x)) row-major, [:,1] = the same
                              image in column-major order (index w*H + h)                          */
    /* backward */
    const float *g2;       /* (B, n_orders, d, H*W) gradient of out2                                      */
    float *gpre;           /* (B, d, H, W) scratch: gradient w.r.t. the pre-activation, fully written -- except for
                              planes with 2 (H + 2) ((W + 2) | 1) 4 <= 48 KiB: one workgroup owns such a plane and
                              keeps gpre in LDS between its two stencils, gpre is then not touched        */
    float *dweight;        /* (d, 1, 3, 3) ACCUMULATED into (caller zeroes); WRITTEN with
                              SIGMA_DWCONV_DETERMINISTIC                                            */
    float *dbias;          /* (d) ACCUMULATED into, or NULL; WRITTEN with SIGMA_DWCONV_DETERMINISTIC */
    float *dx;             /* (B, d, H, W) fully written                                           */
    /* ABI 10: planes of x and dx need not be packed as (B, d): plane (b, c) starts at b * x_batch_stride + c * x_channel_stride
     * floats (each plane H*W contiguous); 0 / 0 = the contiguous (B, d, H, W) tensor.  SS2D hands the x half of in_proj over
     * in CHANNEL-major order (d, B, H, W) -- written transposed by the GEMM epilogue (sigma_gemm.h, t_cols), read here in place. */
    int64_t x_batch_stride, x_channel_stride;
    /* ABI 11: device scratch of >= sigma_dwconv3x3_silu_bwd_workspace_bytes() bytes, 16-byte aligned; read only by the
     * backward with SIGMA_DWCONV_DETERMINISTIC (NULL / 0 otherwise). */
    void *workspace;
    int64_t workspace_bytes;
} sigma_dwconv_params;

/* ABI 11, bit of sigma_dwconv_params.flags: deterministic backward.  Every workgroup stores its dweight / dbias sums to a
 * slot of the workspace with plain stores and one more pass adds the slots in a fixed order: dweight and dbias are fully
 * WRITTEN (no zero fill needed) and bitwise reproducible from run to run. */
#define SIGMA_DWCONV_DETERMINISTIC 1

int sigma_dwconv3x3_silu_fwd(const sigma_dwconv_params *params, void *stream);
int sigma_dwconv3x3_silu_bwd(const sigma_dwconv_params *params, void *stream);
/* Scratch bytes of sigma_dwconv3x3_silu_bwd: 0 without SIGMA_DWCONV_DETERMINISTIC, else 40 bytes per channel and
 * workgroup slot (batch x 32x32 tiles, or batch for a plane below the 48 KiB line of gpre); negative = invalid params.
 * The kernels work on strips of <= 32 rows x <= 128 columns (csrc/dwconv.hip), never more of them than 32x32 tiles: they
 * fill the first batch x strips slots and the fixed-order pass reads only those. */
int64_t sigma_dwconv3x3_silu_bwd_workspace_bytes(const sigma_dwconv_params *params);

/*   sigma_cross_merge_nhwc / sigma_cross_split_nhwc
 *       CrossMerge (vmamba.py:100-108) + the transpose to channels-last in front of out_norm
 *       (vmamba.py:221-224), and its adjoint (CrossMerge.backward = CrossScan, vmamba.py:110-121).
 *       The scan kernels already deliver the flipped directions in natural order, so with the group
 *       order g = 2 * memory_order + flipped:
 *           merge:  nhwc[b,h,w,c] = planes4[b,0,c,hW+w] + planes4[b,1,c,hW+w]
 *                                 + planes4[b,2,c,wH+h] + planes4[b,3,c,wH+h]
 *           split:  planes2[b,0,c,hW+w] = planes2[b,1,c,wH+h] = nhwc[b,h,w,c]                      */
typedef struct sigma_merge_params {
    int32_t batch, channels, height, width;
    const float *planes4;  /* merge in : (B, 4, d, H*W)                       */
    float *planes2;        /* split out: (B, 2, d, H*W)                       */
    float *nhwc;           /* merge out / split in: (B, H, W, d) contiguous   */
} sigma_merge_params;

int sigma_cross_merge_nhwc(const sigma_merge_params *params, void *stream);
int sigma_cross_split_nhwc(const sigma_merge_params *params, void *stream);

/*   sigma_transpose2d
 *       dst[b][c][r] = src[b][r][c] with free row / batch strides (floats): the channels-last ->
 *       channels-first copy in front of the depthwise conv (vmamba.py:1070-1071) reading the x half
 *       of the in_proj output in place, and the inverse copy that puts dx into the x half of the
 *       in_proj gradient (what autograd's chunk() backward does with a strided cat).               */
typedef struct sigma_transpose_params {
    int32_t batch, rows, cols, reserved_;
    const float *src;      /* element (b, r, c) at src[b*src_batch_stride + r*src_row_stride + c] */
    float *dst;            /* element (b, c, r) at dst[b*dst_batch_stride + c*dst_row_stride + r] */
    int64_t src_batch_stride, src_row_stride, dst_batch_stride, dst_row_stride;
} sigma_transpose_params;

int sigma_transpose2d(const sigma_transpose_params *params, void *stream);

/*   sigma_pair_sum_add
 *       acc[o][i] += src[2*o][i] + src[2*o + 1][i]  for o < n_outer, i < inner (contiguous fp32).
 *       Adjoint of reading ONE copy of x for the two directions of a memory order (u_group_shift = 1 in
 *       sigma_scan.h): du of the forward and of the flipped direction are added to the x_proj part of the
 *       gradient in one pass (autograd of the reference's CrossScan does it with flips and adds,
 *       vmamba.py:91-98); replaces two strided torch adds.                                        */
int sigma_pair_sum_add(const float *src, float *acc, int64_t n_outer, int64_t inner, void *stream);

/*   sigma_upsample2x_nhwc
 *       F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) of a contiguous channels-last fp32 tensor
 *       (B, H, W, C) -> (B, 2H, 2W, C) (backward = 0), and its adjoint (backward = 1: `in` is the gradient
 *       (B, 2H, 2W, C), `out` the input gradient (B, H, W, C); height / width are ALWAYS those of the small tensor):
 *       the decoder's UpsampleExpand / FinalUpsample_X4 (models/decoders/MambaDecoder.py:33-51, 76-97).  C % 4 == 0,
 *       16-byte aligned pointers.  Gather formulation in both directions (deterministic, no atomics).           */
int sigma_upsample2x_nhwc(const float *in, float *out, int32_t batch, int32_t height, int32_t width, int32_t channels,
                          int32_t backward, void *stream);

/*   sigma_plane_pool / sigma_plane_scale / sigma_plane_dot / sigma_plane_gate_bwd
 *       ChannelAttention of the decoder's conv branch (vmamba.py:1725-1741; called from ChannelAttentionBlock :1744-1757
 *       inside CVSSDecoderBlock :1800-1805):  y = x * sigmoid(fc(avg_pool(x)) + fc(max_pool(x)))  on contiguous
 *       (B, C, H, W) fp32 activations, seen here as `planes` = B * C planes of `hw` = H * W floats.
 *           pool     : mean[p], max[p], count[p] = number of elements of plane p equal to its max (one pass over x)
 *           scale    : out[p][i] = x[p][i] * scale[p]
 *           dot      : out[p] = sum_i a[p][i] * b[p][i]          (d/d scale of the product: a = dy, b = x)
 *           gate_bwd : dx[p][i] = g[p][i] * scale[p] + dmean[p] / hw + (x[p][i] == max[p] ? dmax[p] / count[p] : 0)
 *       -- the gradient of the max pool is shared by tied maxima, as torch.amax does (the reference's
 *       AdaptiveMaxPool2d routes it to one of them; the two agree wherever the maximum is unique).  A NaN element is the
 *       maximum of its plane, as in both: max[p] = NaN and count[p] = 0 (nothing equals it).  The tiny (2B, C)
 *       squeeze/excite MLP between pool and scale stays with the caller.                                          */
int sigma_plane_pool(const float *x, int64_t planes, int64_t hw, float *mean, float *max, float *count, void *stream);
int sigma_plane_scale(const float *x, const float *scale, float *out, int64_t planes, int64_t hw, void *stream);
int sigma_plane_dot(const float *a, const float *b, float *out, int64_t planes, int64_t hw, void *stream);
typedef struct sigma_gate_bwd_params {
    int64_t planes, hw;
    const float *g;        /* (planes, hw) gradient of the gated output                     */
    const float *x;        /* (planes, hw) input of the gate                                */
    const float *scale;    /* (planes) sigmoid gate of the forward                          */
    const float *dmean;    /* (planes) gradient of the pooled means                         */
    const float *dmax;     /* (planes) gradient of the pooled maxima                        */
    const float *max;      /* (planes) pooled maxima of the forward                         */
    const float *count;    /* (planes) ties of the forward                                  */
    float *dx;             /* (planes, hw) fully written                                    */
} sigma_gate_bwd_params;
int sigma_plane_gate_bwd(const sigma_gate_bwd_params *params, void *stream);

/*   sigma_softmax_ce_fwd / sigma_softmax_ce_bwd
 *       nn.CrossEntropyLoss(reduction='mean', ignore_index) of models/builder.py:146-166 (criterion built in
 *       train.py:95) on channels-last logits: `rows` pixels of `classes` contiguous fp32 logits (classes % 4 == 0,
 *       16-byte aligned), int64 labels.
 *           fwd : lse[r] = log sum_c exp(logit[r][c]);  partial[2k], partial[2k+1] = (sum of lse[r] - logit[r][label[r]],
 *                 number of pixels) over the pixels workgroup k < SIGMA_CE_BLOCKS handled with label != ignore_index
 *                 (labels outside [0, classes) count as ignored; the reference asserts on them).  The caller adds the
 *                 SIGMA_CE_BLOCKS pairs: loss = sum / count, deterministic.
 *           bwd : dlogits[r][c] = (exp(logit[r][c] - lse[r]) - [c == label[r]]) * scale[0], zero for ignored pixels;
 *                 scale = upstream gradient / count, a DEVICE scalar (no host synchronisation).                   */
#define SIGMA_CE_BLOCKS 1024
int sigma_softmax_ce_fwd(const float *logits, const int64_t *labels, int64_t rows, int32_t classes, int64_t ignore_index,
                         float *lse, float *partial, void *stream);
int sigma_softmax_ce_bwd(const float *logits, const int64_t *labels, const float *lse, const float *scale, int64_t rows,
                         int32_t classes, int64_t ignore_index, float *dlogits, void *stream);
/*   sigma_softmax_ce_fwd_ld / sigma_softmax_ce_bwd_ld (added under ABI 13: two functions, no struct or signature changed)
 *       The same loss for ANY class count (the reference's MFNet 9, PST900 5, SUN-RGBD 37): row r holds its `classes`
 *       logits at logits + r * ld, with the pitch ld % 4 == 0, ld >= classes, classes >= 1 and 16-byte aligned pointers --
 *       the (rows, ld) output of the classifier GEMM against a weight zero-padded to ld rows.  `dlogits` has the same
 *       pitch.  ld == classes IS sigma_softmax_ce_fwd / _bwd (same kernels, same bits).
 *           fwd : columns >= classes take no part; they may hold anything (NaN, Inf) and reach neither lse nor partial.
 *                 lse and the SIGMA_CE_BLOCKS (sum, count) pairs are laid out as above.
 *           bwd : columns < classes as above; columns [classes, ld) are WRITTEN with exact zeros (chosen by index), so
 *                 GEMMs may read whole rows of ld.
 *       A label in [classes, ld) is out of range like any label >= classes: the pixel is ignored.
 *       Rows of up to 64 classes (16 chunks of 16 bytes) are held in registers, longer ones are walked.
 *       Non-finite logits, for every entry point of the family (plain, option, focal; both forms, either pitch):
 *           a -inf logit away from the label is a MASKED CLASS: it adds exp(-inf) = 0 to the sum, lse and the loss are
 *           those of the remaining classes and its dlogit is exactly zero -- wherever it sits, a first 16-byte chunk that
 *           is masked whole included (without label smoothing: the smoothing term sums w_c x_c over every class);
 *           a row that holds NaN or +inf, is -inf throughout or has -inf at its label touches only ITS OWN lse, row_loss
 *           and dlogits row -- every other row keeps its bits -- and reaches the partial pair of its workgroup only if
 *           it is labelled: an ignored row adds nothing, whatever it holds.  lse of such a row is non-finite exactly
 *           where logsumexp is; -inf at the label gives a finite lse and row_loss = +inf.  The gradient values inside
 *           such a row are not specified; the pad columns are exact zeros all the same.                             */
int sigma_softmax_ce_fwd_ld(const float *logits, const int64_t *labels, int64_t rows, int32_t classes, int32_t ld,
                            int64_t ignore_index, float *lse, float *partial, void *stream);
int sigma_softmax_ce_bwd_ld(const float *logits, const int64_t *labels, const float *lse, const float *scale, int64_t rows,
                            int32_t classes, int32_t ld, int64_t ignore_index, float *dlogits, void *stream);

/*   sigma_softmax_ce_opt_fwd / sigma_softmax_ce_opt_bwd (added under ABI 13: two functions and their own struct, no existing
 *   struct or signature changed -- the version counts changes to what a caller built against an older header relies on)
 *       Every option of nn.CrossEntropyLoss on the same rows: class weights w (all ones when NULL), label smoothing eps,
 *       reduction 'mean' / 'sum' / 'none', ignore_index.  With W = sum_c w_c, p = softmax(logits[r]), y = labels[r] and
 *       "valid" as above (y != ignore_index and 0 <= y < classes):
 *           fwd : lse[r] as above;
 *                 row_loss[r] = (1 - eps) w_y (lse - x_y) + (eps / classes) sum_c w_c (lse - x_c)  for valid rows, 0 otherwise
 *                 (written when row_loss != NULL: reduction 'none');
 *                 partial[2k], partial[2k+1] = (sum of row_loss, sum of w_y) over the valid rows of workgroup k <
 *                 SIGMA_CE_BLOCKS, in the fixed order of the plain kernels.  'sum' = sum of partial[2k]; 'mean' = that over
 *                 the sum of partial[2k+1] (the pixel count when there is no weight).
 *           bwd : dlogits[r][c] = g_r [ (1 - eps) w_y (p_c - [c == y]) + (eps / classes) (W p_c - w_c) ]  for valid rows,
 *                 exact zeros otherwise and in columns [classes, ld).  g_r = scale[0], a DEVICE scalar (upstream / sum of
 *                 w_y for 'mean', upstream for 'sum'), or row_grad[r] ('none'): exactly one of the two is non-NULL.
 *       Pitch, padding, alignment and the two regimes (row in registers up to 64 classes) are those of the _ld entry
 *       points; the weight is read through the caches (4-byte aligned, `classes` floats), it gets no gradient.
 *       SIGMA_OPS_ERR_ARG before any launch: classes < 1, ld % 4 != 0, ld < classes, rows < 0, label_smoothing outside
 *       [0, 1], a misaligned pointer, a missing required pointer, both or neither of scale and row_grad.              */
typedef struct sigma_ce_opt_params {
    int64_t rows;
    int32_t classes, ld;           /* ld % 4 == 0, ld >= classes >= 1                                      */
    int64_t ignore_index;
    float label_smoothing;         /* eps in [0, 1]                                                        */
    int32_t reserved_;
    const float *logits;           /* row r at logits + r * ld, 16-byte aligned                            */
    const int64_t *labels;         /* (rows)                                                               */
    const float *weight;           /* (classes) or NULL = all ones                                         */
    float *lse;                    /* (rows): fwd out, bwd in                                              */
    float *row_loss;               /* fwd out (rows), or NULL                                              */
    float *partial;                /* fwd out: SIGMA_CE_BLOCKS pairs (sum of row_loss, sum of w_y)         */
    const float *scale;            /* bwd in: device scalar g, or NULL                                     */
    const float *row_grad;         /* bwd in: (rows) g_r, or NULL                                          */
    float *dlogits;                /* bwd out: pitch ld, 16-byte aligned, fully written                    */
} sigma_ce_opt_params;
int sigma_softmax_ce_opt_fwd(const sigma_ce_opt_params *params, void *stream);
int sigma_softmax_ce_opt_bwd(const sigma_ce_opt_params *params, void *stream);

/*   sigma_softmax_focal_fwd / sigma_softmax_focal_bwd  (additions only: the struct above as it is, the ABI version stays 13)
 *       The focal loss of FocalLoss2d (utils/loss_opr.py:12-23) on the same rows, with a run-time exponent `gamma`.  With
 *       p = softmax(logits[r]), y = labels[r], q = 1 - p_y, nll = lse - x_y and "valid" as above:
 *           fwd : lse[r] as above;
 *                 row_loss[r] = w_y q^gamma nll  for valid rows, 0 otherwise (written when row_loss != NULL);
 *                 partial = SIGMA_CE_BLOCKS pairs (sum of row_loss, sum of w_y), workgroups and row order of the option
 *                 kernels.  'mean' = sum of partial[2k] over sum of partial[2k+1], what nn.NLLLoss(weight, 'mean') gives.
 *           bwd : dlogits[r][c] = g_r w_y m (p_c - [c == y]),   m = q^gamma + gamma q^(gamma - 1) p_y nll,
 *                 for valid rows, exact zeros otherwise and in columns [classes, ld); q, nll and m are formed again from
 *                 the row and the saved lse.  g_r = scale[0] or row_grad[r] as above.  No atomics, nothing read back.
 *       gamma is 0 (the cross entropy) or >= 1; gamma = 2, the reference's fixed exponent, is a plain square.  For
 *       0 < gamma < 1 the factor q^(gamma - 1) is unbounded as p_y -> 1 and fp32 rows cannot bound the error of m: refused.
 *       Where q = 0 in fp32 (the label's logit dominates) the row's loss is exactly 0 and, for gamma > 0, its gradient row
 *       is exact zeros; for gamma = 0 it is the cross-entropy row.
 *       SIGMA_OPS_ERR_ARG before any launch: everything the option entry points refuse, label_smoothing != 0, gamma NaN,
 *       infinite, negative or in (0, 1).                                                                            */
int sigma_softmax_focal_fwd(const sigma_ce_opt_params *params, float gamma, void *stream);
int sigma_softmax_focal_bwd(const sigma_ce_opt_params *params, float gamma, void *stream);

/*   sigma_ohem_select / sigma_ohem_workspace_bytes  (csrc/ohem.hip; additions only, the ABI version stays 13)
 *       the pixel selection of ProbOhemCrossEntropy2d (utils/loss_opr.py:137-187) on the device, in the negative-log
 *       domain.  `nll` holds lse - x_y per row, as sigma_softmax_ce_opt_fwd writes it to row_loss with weight = NULL and
 *       label_smoothing = 0 (0 at ignored rows).  A row is VALID when label != ignore_index and 0 <= label < classes.
 *         no mining   min_kept <= 0, num_valid == 0 or min_kept > num_valid:  tau = -inf, every valid row is kept
 *                     (thresh is not applied, as in the reference)
 *         mining      tau = min((float)(0.0 - log((double)thresh)), the min_kept-th LARGEST nll of the valid rows);
 *                     a valid row is kept unless nll < tau: ties at tau are all kept, and so is a NaN key
 *       Out:  tau[0];  counts[0] = num_valid, counts[1] = kept rows;  mined[r] = labels[r] if the row is kept, else
 *       ignore_index.  With `weight` / `row_loss` / `partial` (each optional) also what sigma_softmax_ce_opt_fwd would
 *       give for (mined, weight, label_smoothing = 0) without reading the logits again: row_loss[r] = w_y nll[r] at kept
 *       rows and 0 elsewhere, partial = SIGMA_CE_BLOCKS pairs (sum of row_loss, sum of w_y) in that kernel's row order --
 *       the same bits.
 *       The k-th value comes from a radix select, four 8-bit digits of the order-preserving unsigned image of the keys:
 *       per pass up to SIGMA_OHEM_HIST_BLOCKS workgroups count into LDS and add their non-empty bins to a global
 *       histogram with integer atomics (exact in any order: the result is bitwise reproducible), one workgroup picks the
 *       digit.  Ten kernels, all launched unconditionally; nothing is read back, so the call can be
 *       captured into a graph and the branch taken at replay is the data's.  The logits are not touched: each pass
 *       reads 4-byte keys and 8-byte labels.
 *       rows == 0 is a success that writes tau = -inf and counts = (0, 0) (nll, labels, mined may be NULL then).
 *       SIGMA_OPS_ERR_ARG before any launch: a NULL params, tau, counts or workspace, a NULL nll / labels / mined with
 *       rows > 0, a misaligned pointer (floats 4, labels / mined / counts 8, workspace 16 bytes), workspace_bytes below
 *       sigma_ohem_workspace_bytes(rows), thresh outside (0, 1] (NaN included), classes < 1, rows < 0 or above 2^31 - 1.
 *       The size query answers a multiple of 16 that does not shrink as rows grow, and -1 for rows it refuses.         */
#define SIGMA_OHEM_HIST_BLOCKS 512
typedef struct sigma_ohem_params {
    int64_t rows;
    int64_t ignore_index;
    int32_t classes;               /* labels outside [0, classes) count as ignored                           */
    float thresh;                  /* in (0, 1]                                                              */
    int64_t min_kept;
    const float *nll;              /* (rows) keys                                                            */
    const int64_t *labels;         /* (rows)                                                                 */
    int64_t *mined;                /* out (rows)                                                             */
    float *tau;                    /* out (1)                                                                */
    int64_t *counts;               /* out (2): num_valid, kept                                               */
    void *workspace;               /* 16-byte aligned scratch; its contents on entry do not matter           */
    int64_t workspace_bytes;
    const float *weight;           /* (classes) or NULL = all ones                                           */
    float *row_loss;               /* out (rows), or NULL                                                    */
    float *partial;                /* out: SIGMA_CE_BLOCKS pairs, or NULL                                    */
} sigma_ohem_params;
int sigma_ohem_select(const sigma_ohem_params *params, void *stream);
int64_t sigma_ohem_workspace_bytes(int64_t rows);

/*   sigma_upsample_ce_fwd / sigma_upsample_ce_bwd  (csrc/deepsup.hip; additions only, the ABI version stays 13)
 *       The plain kind of the one forward and the one backward kernel template that also serve sigma_upsample_loss_* below.
 *       nn.CrossEntropyLoss(reduction='mean', ignore_index) of the bilinear x `scale` upsampling (align_corners=False) of
 *       COARSE channels-last logits: the loss of the deep-supervision heads of MambaDecoder (models/decoders/
 *       MambaDecoder.py:264-270, models/builder.py:158-166) with the bias-free 1x1 head run BEFORE the interpolation -- the
 *       two commute.  The interpolated row z^ of `classes` logits of a fine pixel is formed on the fly, never stored.
 *       Per axis, with n the coarse size (height for rows, width for columns) and s = scale:
 *           src = max((dst + 0.5) / s - 0.5, 0),  i0 = floor(src),  i1 = min(i0 + 1, n - 1),  lambda = src - i0
 *       (evaluated in integers: exact taps for every s, exact weights for s a power of two).
 *           fwd : one fine pixel per thread, rows in the order of the plain kernels: lse[P] = logsumexp(z^(P)); a valid pixel
 *                 (label != ignore_index, 0 <= label < classes) adds lse - z^_y and 1 to its workgroup's pair of `partial`
 *                 (SIGMA_CE_BLOCKS pairs, all written).  Columns >= classes of the coarse rows take no part; they may hold NaN.
 *           bwd : dlogits[b, i, j, c] = g * sum over the valid fine pixels P of wgt(P -> (i, j)) (exp(z^_c(P) - lse(P)) - [c == y(P)]),
 *                 g = scale_grad[0] (upstream / count, a DEVICE scalar).  Gather: the lanes that own (b, i, j) and a chunk of
 *                 four classes walk the footprint of the coarse pixel in a fixed order with the forward's index function (at a
 *                 border i0 == i1 and both weights land on the same pixel).  No atomics, bitwise reproducible; columns
 *                 [classes, ld) are written with exact zeros, the buffer is fully written.
 *       SIGMA_OPS_ERR_ARG before any launch: classes < 1 or > 64, ld % 4 != 0, ld < classes, scale outside [1, 32], a
 *       non-positive size, more than 2^31 - 1 fine pixels, a missing or misaligned pointer (logits / dlogits 16 bytes, labels
 *       8, the rest 4; fwd needs partial, bwd scale_grad and dlogits).                                                  */
typedef struct sigma_upsample_ce_params {
    int32_t batch, height, width;  /* of the COARSE logits                                                   */
    int32_t scale;                 /* s in [1, 32]: fine size (height * s, width * s)                        */
    int32_t classes, ld;           /* ld % 4 == 0, ld >= classes, 1 <= classes <= 64                         */
    int64_t ignore_index;
    const float *logits;           /* coarse pixel (b, i, j) at logits + ((b * height + i) * width + j) * ld */
    const int64_t *labels;         /* (batch, height * s, width * s)                                         */
    float *lse;                    /* one float per fine pixel: fwd out, bwd in                              */
    float *partial;                /* fwd out: SIGMA_CE_BLOCKS pairs (sum, count)                            */
    const float *scale_grad;       /* bwd in: device scalar g                                                */
    float *dlogits;                /* bwd out: coarse, pitch ld, fully written                               */
} sigma_upsample_ce_params;
int sigma_upsample_ce_fwd(const sigma_upsample_ce_params *params, void *stream);
int sigma_upsample_ce_bwd(const sigma_upsample_ce_params *params, void *stream);

/*   sigma_upsample_loss_fwd / sigma_upsample_loss_bwd  (csrc/deepsup.hip; additions only -- a struct and two functions of
 *   their own, nothing above changes -- the ABI version stays 13)
 *       The criteria with options on the same interpolated rows z^ (geometry, index function, pad and validity as for
 *       sigma_upsample_ce_*: further kinds of the same two kernel templates, which apply the upstream gradient per fine
 *       pixel where the plain kind scales the finished sum once): with l = lse(z^(P)), p = softmax(z^(P)), y = labels[P],
 *       w the class weights (all ones when NULL), W = sum_c w_c,
 *         kind SIGMA_UPSAMPLE_LOSS_OPTIONS   the row formulas of sigma_softmax_ce_opt_*:
 *           row_loss[P] = (1 - eps) w_y (l - z^_y) + (eps / classes) (W l - sum_c w_c z^_c)
 *           d row_loss / d z^_c = (1 - eps) w_y (p_c - [c == y]) + (eps / classes) (W p_c - w_c)
 *         kind SIGMA_UPSAMPLE_LOSS_FOCAL     those of sigma_softmax_focal_* (q = 1 - p_y, nll = l - z^_y):
 *           row_loss[P] = w_y q^gamma nll,   d row_loss / d z^_c = w_y m (p_c - [c == y]),  m = q^gamma + gamma q^(gamma - 1) p_y nll
 *           fwd : lse[P]; row_loss[P] for valid pixels and 0 otherwise (written when row_loss != NULL: reduction 'none', and --
 *                 OPTIONS with weight = NULL and eps = 0 -- the nll that sigma_ohem_select takes); FOCAL also writes
 *                 coef[P] = w_y m(P) (0 at pixels that are not valid); partial = SIGMA_CE_BLOCKS pairs (sum of row_loss, sum
 *                 of w_y), workgroups and pixel order of sigma_upsample_ce_fwd, all written.
 *           bwd : dlogits[b, i, j, c] = sum over the valid fine pixels P of wgt(P -> (i, j)) g_P d row_loss(P) / d z^_c(P), the
 *                 gather of sigma_upsample_ce_bwd (same lanes per item, same butterfly; no atomics, bitwise reproducible,
 *                 exact zeros in columns [classes, ld), fully written).  g_P = scale_grad[0], a DEVICE scalar (upstream / sum
 *                 of w_y for 'mean', upstream for 'sum'), or row_grad[P] ('none'): exactly one of the two is non-NULL.  FOCAL
 *                 reads coef and lse as the forward wrote them and does not gather the label's column again.  OHEM: the
 *                 backward of OPTIONS on the mined labels.
 *       SIGMA_OPS_ERR_ARG before any launch: everything sigma_upsample_ce_* refuses on the geometry, a kind other than the
 *       two, label_smoothing outside [0, 1] (NaN included) or non-zero with FOCAL, gamma (FOCAL only) NaN, infinite, negative
 *       or in (0, 1), a missing or misaligned pointer (logits / dlogits 16 bytes, labels 8, the rest 4; both directions need
 *       logits, labels, lse and, with FOCAL, coef; fwd needs partial, bwd dlogits), both or neither of scale_grad and
 *       row_grad in the backward.                                                                                       */
#define SIGMA_UPSAMPLE_LOSS_OPTIONS 0
#define SIGMA_UPSAMPLE_LOSS_FOCAL 1
typedef struct sigma_upsample_loss_params {
    int32_t batch, height, width;  /* of the COARSE logits                                                   */
    int32_t scale;                 /* s in [1, 32]: fine size (height * s, width * s)                        */
    int32_t classes, ld;           /* ld % 4 == 0, ld >= classes, 1 <= classes <= 64                         */
    int64_t ignore_index;
    int32_t kind;                  /* SIGMA_UPSAMPLE_LOSS_OPTIONS or SIGMA_UPSAMPLE_LOSS_FOCAL               */
    float label_smoothing;         /* eps in [0, 1]; 0 with FOCAL                                            */
    float gamma;                   /* FOCAL: 0 or >= 1; not read otherwise                                   */
    int32_t reserved_;
    const float *logits;           /* coarse pixel (b, i, j) at logits + ((b * height + i) * width + j) * ld */
    const int64_t *labels;         /* (batch, height * s, width * s)                                         */
    const float *weight;           /* (classes) or NULL = all ones                                           */
    float *lse;                    /* one float per fine pixel: fwd out, bwd in                              */
    float *row_loss;               /* fwd out, one float per fine pixel, or NULL                             */
    float *coef;                   /* FOCAL: one float per fine pixel, fwd out, bwd in; not touched otherwise */
    float *partial;                /* fwd out: SIGMA_CE_BLOCKS pairs (sum of row_loss, sum of w_y)           */
    const float *scale_grad;       /* bwd in: device scalar g, or NULL                                       */
    const float *row_grad;         /* bwd in: g_P per fine pixel, or NULL                                    */
    float *dlogits;                /* bwd out: coarse, pitch ld, fully written                               */
} sigma_upsample_loss_params;
int sigma_upsample_loss_fwd(const sigma_upsample_loss_params *params, void *stream);
int sigma_upsample_loss_bwd(const sigma_upsample_loss_params *params, void *stream);

/*   sigma_colscale_bwd
 *       backward of  y = a + x * scale with a per-channel `scale` on contiguous channels-last rows (rows, C): the residual
 *       of the decoder block, x * scale1 + op(norm1(x)) and x * scale2 + conv_blk(norm2(x)) (vmamba.py:1800-1805):
 *           dx[r][c] = dy[r][c] * scale[c]          dscale[c] += sum_r dy[r][c] * x[r][c]
 *       in one pass over dy and x (the autograd formulation: two multiplies and a column reduction).  `dscale` is
 *       ZERO-FILLED by the caller (float atomics, one per block and channel).  C % 4 == 0, C <= 1024, 16-byte aligned
 *       operands.                                                                                                   */
int sigma_colscale_bwd(const float *dy, const float *x, const float *scale, float *dx, float *dscale, int64_t rows,
                       int32_t channels, void *stream);
/*   sigma_colscale_bwd_ws (ABI 11)
 *       the same backward with dscale fully WRITTEN through a deterministic two-stage sum: every block stores its column
 *       sums to a row of `workspace` (>= sigma_colscale_bwd_workspace_bytes(rows, channels) bytes, 16-byte aligned), a
 *       second pass adds the rows in a fixed order.  Bitwise reproducible; no zero fill of dscale.  The size query returns
 *       a negative value for invalid sizes.                                                                           */
int sigma_colscale_bwd_ws(const float *dy, const float *x, const float *scale, float *dx, float *dscale, int64_t rows,
                          int32_t channels, void *workspace, int64_t workspace_bytes, void *stream);
int64_t sigma_colscale_bwd_workspace_bytes(int64_t rows, int32_t channels);

/*   sigma_layernorm_fwd / sigma_layernorm_bwd
 *       nn.LayerNorm(C, eps=1e-5, affine) over the last dimension of a contiguous (rows, C) fp32
 *       tensor: every LayerNorm of the hot path (vmamba.py:617, 724, 1183-1184, 1448-1449, 1693,
 *       1783, 1797; MambaDecoder.py:18, 41, 85).  C % 4 == 0, C <= 2048.
 *       bwd: dx fully written; dgamma / dbeta fully written (deterministic two-stage column sums
 *       through `workspace` of sigma_layernorm_bwd_partial_rows(rows, C) * 2 * C floats).
 *       bwd with a gate needs beta as well (the normalised value is recomputed).                  */
typedef struct sigma_layernorm_params {
    int64_t rows;
    int32_t channels;
    float eps;
    const float *x;        /* (rows, C)                       */
    const float *gamma;    /* (C)                             */
    const float *beta;     /* (C) or NULL                     */
    float *y;              /* fwd out (rows, C)               */
    float *mean;           /* fwd out / bwd in (rows), or NULL in a forward that needs no backward */
    float *rstd;           /* fwd out / bwd in (rows)         */
    const float *dy;       /* bwd in  (rows, C)               */
    float *dx;             /* bwd out (rows, C)               */
    float *dgamma;         /* bwd out (C)                     */
    float *dbeta;          /* bwd out (C) or NULL             */
    float *workspace;      /* bwd scratch                     */
    /* optional fused gate of SS2D.forward (vmamba.py:1077: y = out_norm(y) * act(z)):
     * y = LayerNorm(x) * silu(gate);  gate rows are gate_row_stride floats apart (z is the second
     * half of the in_proj output); dgate rows are dgate_row_stride floats apart (0 = C, contiguous):
     * the caller can have dz written straight into the z half of the in_proj output's gradient.
     * NULL gate = plain LayerNorm.  */
    const float *gate;
    int64_t gate_row_stride;
    float *dgate;
    int64_t dgate_row_stride;
    /* optional per-sample factor on the OUTPUT (stochastic depth, timm DropPath as used by VSSBlock vmamba.py:1716-1722
     * and CVSSDecoderBlock :1800-1805: the branch is multiplied by mask[b] / keep_prob before the residual add):
     * y = (LayerNorm(x) [* silu(gate)]) * row_scale[r / rows_per_scale]; the backward multiplies dy by the same factor
     * on load.  The out_proj that follows is linear and bias-free, so scaling its input scales the branch.  NULL = 1. */
    const float *row_scale;
    int64_t rows_per_scale;
    /* ABI 8: optional addend of dx, (rows, C) contiguous, 16-byte aligned (may be dx itself): the gradient that reached x
     * on the path AROUND the LayerNorm -- the residual stream of a block, x + op(norm(x)) (vmamba.py:1716-1722) --
     * joined here instead of in an add pass of its own.  Backward only; NULL = none. */
    const float *dx_add;
} sigma_layernorm_params;

int sigma_layernorm_fwd(const sigma_layernorm_params *params, void *stream);
int sigma_layernorm_bwd(const sigma_layernorm_params *params, void *stream);
/* rows of 2 * C floats the backward needs in `workspace`: one partial (dgamma, dbeta) row per WORKGROUP (its four waves
 * meet in LDS), added up in a fixed order by a second small kernel */
int sigma_layernorm_bwd_partial_rows(int64_t rows, int32_t channels);

/* ---- evaluation: multi-scale score sum, arg-max and confusion matrix (csrc/segmetric.hip) ----
 *
 * The reference's evaluator (engine/evaluator.py:433-450, utils/metric.py:8-15) adds the (H, W, C) float32 scores of
 * every scale into a float64 array, takes argmax(2) and counts hist[gt * n_cl + pred] over the pixels with
 * 0 <= gt < n_cl.  Scores are held class-planar here, (C, pixels): the layout the evaluator's device score already
 * has before its permute to (H, W, C), and the one in which a lane per pixel reads every class plane coalesced.
 * Both entry points reproduce the host result exactly: the same IEEE float64 adds in the same (scale) order, numpy's
 * arg-max rules, integer counts. */
typedef struct sigma_seg_accumulate_params {
    int64_t pixels;                /* pixels per class plane (H * W)                                         */
    int32_t classes;               /* C >= 1                                                                 */
    int32_t first;                 /* 1: acc = 0.0 + (double)score -- numpy's np.zeros(...) += score, so no
                                      zero fill is needed (and -0.0 becomes +0.0 as it does there);
                                      0: acc += (double)score                                               */
    const float *score;            /* class plane c at score + c * score_plane_stride, pixels contiguous     */
    double *acc;                   /* class plane c at acc + c * acc_plane_stride                            */
    int64_t score_plane_stride;    /* elements; >= pixels                                                    */
    int64_t acc_plane_stride;      /* elements; >= pixels                                                    */
} sigma_seg_accumulate_params;

int sigma_seg_accumulate(const sigma_seg_accumulate_params *params, void *stream);

typedef struct sigma_seg_confusion_params {
    int64_t pixels;                /* pixels of the image (H * W), < 2^31                                    */
    int32_t classes;               /* C planes of `acc` (1..65535), or 0 when `acc` is NULL                  */
    int32_t n_cl;                  /* 1..256: hist is n_cl x n_cl                                            */
    int32_t gt_elem_size;          /* 1: uint8 labels, 8: int64 labels                                       */
    int32_t pred_elem_size;        /* 1: uint8, 8: int64 (numpy's argmax dtype); 1 needs classes <= 256      */
    const double *acc;             /* the summed scores, class plane c at acc + c * acc_plane_stride; NULL:
                                      `pred` is an INPUT (hist_info of a given prediction)                   */
    int64_t acc_plane_stride;      /* elements; >= pixels                                                    */
    void *pred;                    /* (pixels,) arg-max over the classes, first maximum / first NaN wins
                                      (numpy's argmax); written when acc != NULL (NULL = not written),
                                      read when acc == NULL                                                  */
    const void *gt;                /* (pixels,) labels; a pixel counts when 0 <= gt < n_cl (255 = ignore);
                                      NULL = arg-max only (pred required, hist / counts unused)              */
    int64_t *hist;                 /* (n_cl, n_cl) row gt, column pred; counts are ADDED (zero it first)     */
    int64_t *counts;               /* [labeled, correct, invalid], ADDED; invalid = counted pixels whose pred
                                      is outside [0, n_cl) -- they are not binned                           */
} sigma_seg_confusion_params;

/* per-workgroup uint32 histograms in LDS when n_cl * n_cl * 4 <= SIGMA_SEG_LDS_HIST_BYTES (n_cl <= 90), flushed into
 * the int64 global histogram; above that, int64 atomics straight into the global histogram.  Integer adds only: the
 * result is exact and the same in any order. */
#define SIGMA_SEG_LDS_HIST_BYTES 32768
int sigma_seg_argmax_confusion(const sigma_seg_confusion_params *params, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGMA_OPS_H_ */
