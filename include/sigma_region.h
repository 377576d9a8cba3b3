/*
 * sigma_region.h -- C ABI of the soft region-overlap losses (Dice, Jaccard, Tversky) in libsigma_hip.so.
 *
 * A criterion of the project's own (the reference trains with per-pixel losses only): the overlap score the evaluator
 * reports, made differentiable, optionally summed with the mean cross entropy.  Kernels: csrc/region.hip.
 *
 * Same conventions as sigma_ops.h: device pointers, float32 rows, the callee enqueues on `stream` (hipStream_t as void*)
 * of the current device, never allocates, never synchronises; returns SIGMA_OPS_OK or a SIGMA_OPS_ERR_* code
 * (sigma_ops.h), and every non-zero status and every -1 of the size query leaves its reason in the error text read with
 * sigma_scan_last_error() (sigma_scan.h).
 *
 * Rows: row r is logits + r * ld, `classes` logits x, ld % 4 == 0, ld >= classes, 1 <= classes <= 64 (a row is held in
 * registers); columns [classes, ld) are never read as values and may hold NaN.  labels are int64.  A row is VALID when
 * label != ignore_index and 0 <= label < classes (the rule of the loss family, sigma_ops.h).
 *
 * With p = softmax(x) and sums over the valid rows:
 *     I_c = sum p_c [y = c]      P_c = sum p_c      Y_c = sum [y = c]      n = number of valid rows
 *     N_c = I_c + s              D_c = (1 - a - b) I_c + a P_c + b Y_c + s              T_c = N_c / D_c
 *     K = { c : Y_c > 0 }        region = (1 / |K|) sum_{c in K} (1 - T_c)              (0 when K is empty)
 *     loss = region_weight region + ce_weight (1 / n) sum_valid (lse - x_y)             (CE term 0 when n = 0)
 * Tversky has (a, b) = (alpha, beta); Dice is a = b = 0.5, Jaccard a = b = 1.  s = smooth >= 0; s = 0 is legal because
 * D_c >= b Y_c > 0 for every class of K (b > 0 and a >= 0 are required).
 *
 *   sigma_region_loss_fwd    three steps on `stream`, no atomics, no host read-back:
 *       sums   SIGMA_CE_BLOCKS workgroups walk the rows: lse[r] for every row; for valid rows p_c = exp(x_c - lse) is added
 *              to the thread's P_c, and to I_y and Y_y of the label; per class the workgroup's threads meet in a fixed order
 *              (wave, then the four waves) and the workgroup writes its slot of 3 classes + 2 floats of `workspace`:
 *              I, P, Y, sum of lse - x_y, number of valid rows.  A -inf logit away from the label is a masked class (p = 0).
 *       coef   one workgroup adds the slots in a fixed order in fp64 and writes
 *              loss[0];  terms[0] = region, terms[1] = the mean cross entropy (both unweighted);
 *              sums[0 .. 3 classes) = I, P, Y as fp32;
 *              coef[c] = A_c = dloss / dI_c = -(rw / |K|) (D_c - (1 - a - b) N_c) / D_c^2,
 *              coef[classes + c] = B_c = dloss / dP_c = (rw / |K|) a N_c / D_c^2      (both 0 outside K),
 *              coef[2 classes] = ce_weight / n (0 when n = 0).
 *   sigma_region_loss_bwd    one pass: with g_c = B_c + A_c [c = y], dot = sum_c p_c g_c and G = scale[0],
 *              dlogits[r][c] = G [ p_c (g_c - dot) + coef[2 classes] (p_c - [c = y]) ]    for valid rows,
 *              exact zeros for the other rows and in columns [classes, ld), chosen by index.  Reads logits, labels, lse
 *              and coef as the forward left them.  rows == 0: nothing is launched.
 *   sigma_region_loss_workspace_bytes    the bytes of `workspace` the forward needs (a function of `classes` alone), or -1
 *              for parameters the launches refuse on their values (pointers are not looked at).
 *
 * SIGMA_OPS_ERR_ARG before any launch: NULL params; classes < 1 or > 64; ld % 4 != 0 or ld < classes; rows < 0;
 * beta <= 0, alpha < 0, smooth < 0, a negative region_weight or ce_weight (NaN fails each); a missing pointer (logits,
 * labels and lse only when rows > 0); logits / dlogits off a 16-byte boundary, labels off 8, any other off 4; a workspace
 * smaller than the query's answer.
 */
#ifndef SIGMA_REGION_H_
#define SIGMA_REGION_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sigma_region_params {
    int64_t rows;
    int32_t classes, ld;
    int64_t ignore_index;
    double alpha, beta;            /* a, b of the Tversky index                                              */
    double smooth;                 /* s                                                                      */
    double region_weight, ce_weight;
    const float *logits;           /* (rows, ld)                                                             */
    const int64_t *labels;         /* (rows)                                                                 */
    float *lse;                    /* (rows): fwd out, bwd in                                                */
    void *workspace;               /* fwd scratch: sigma_region_loss_workspace_bytes                         */
    int64_t workspace_bytes;
    float *loss;                   /* fwd out (1)                                                            */
    float *terms;                  /* fwd out (2): region, mean cross entropy                                */
    float *coef;                   /* (2 classes + 1): fwd out, bwd in                                       */
    float *sums;                   /* fwd out (3 classes): I, P, Y                                           */
    const float *scale;            /* bwd in (1): the upstream gradient G                                    */
    float *dlogits;                /* bwd out (rows, ld), every element written                              */
} sigma_region_params;

int sigma_region_loss_fwd(const sigma_region_params *params, void *stream);
int sigma_region_loss_bwd(const sigma_region_params *params, void *stream);
int64_t sigma_region_loss_workspace_bytes(const sigma_region_params *params);

#ifdef __cplusplus
}
#endif

#endif /* SIGMA_REGION_H_ */
