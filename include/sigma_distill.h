/*
 * sigma_distill.h -- C ABI of the distillation loss (temperature KL against a teacher + cross entropy) in libsigma_hip.so.
 *
 * A criterion of the project's own (the reference trains every model size alone): the student's logits are held to the
 * frozen teacher's at temperature T, optionally summed with the mean cross entropy.  Kernels: csrc/distill.hip.
 *
 * Same conventions as sigma_ops.h: device pointers, float32 rows, the callee enqueues on `stream` (hipStream_t as void*)
 * of the current device, never allocates, never synchronises; returns SIGMA_OPS_OK or a SIGMA_OPS_ERR_* code
 * (sigma_ops.h), and every non-zero status and every -1 of the size query leaves its reason in the error text read with
 * sigma_scan_last_error() (sigma_scan.h).
 *
 * Rows: row r of the student is logits + r * ld, of the teacher teacher + r * ld_t: `classes` logits x and t, both
 * pitches % 4 == 0 and >= classes, 1 <= classes <= 64 (both rows are held in registers); columns [classes, ld) and
 * [classes, ld_t) are never read as values and may hold NaN.  labels are int64.  A row is VALID when label != ignore_index
 * and 0 <= label < classes (the rule of the loss family, sigma_ops.h); n = the number of valid rows.  The KD set S is the
 * valid rows when kd_all == 0 and every row otherwise.
 *
 * With T = temperature, lp(v)_c = v_c / T - lse(v / T), p = exp(lp(x)), q = exp(lp(t)) and P1 = softmax(x):
 *     kl_r = sum_c [q_c > 0] q_c (lp(t)_c - lp(x)_c)
 *     kd   = T^2 (1 / |S|) sum_{r in S} kl_r                          (0 when S is empty)
 *     ce   = (1 / n) sum_valid (lse(x) - x_y)                         (0 when n = 0)
 *     loss = kd_weight kd + ce_weight ce
 * v / T is formed as v * (float)(1 / T), and lp(t), lp(x) by one and the same instruction sequence: a teacher row whose
 * bits equal the student's gives kl_r == 0.0 and p_c - q_c == 0.0 exactly.  A class with q_c == 0 (a -inf teacher logit)
 * contributes exactly 0, by a select; a -inf student logit at a class with q_c > 0 gives kl_r = +inf (as F.kl_div; the loss
 * is then +inf, or NaN = 0 * inf with kd_weight == 0) and a finite gradient.  The teacher receives no gradient.
 *
 *   sigma_distill_loss_fwd    two steps on `stream`, no atomics, no host read-back:
 *       sums   SIGMA_CE_BLOCKS workgroups walk the rows: lse[3 r + 0 .. 2] = lse(x), lse(x / T), lse(t / T) for every row;
 *              kl_r joins the thread's sum for the rows of S, lse(x) - x_y for the valid rows, with both counts; the
 *              workgroup's threads meet in a fixed order (wave, then the four waves) and the workgroup writes its slot of 4
 *              floats of `workspace`: sum kl, |S|, sum of lse - x_y, n.
 *       coef   one workgroup adds the slots in a fixed order in fp64 and writes
 *              loss[0];  terms[0] = kd, terms[1] = ce (both unweighted);
 *              coef[0] = kd_weight T / |S|, coef[1] = ce_weight / n (each 0 when its count is 0).
 *   sigma_distill_loss_bwd    one pass: with G = scale[0],
 *              dlogits[r][c] = G ( [r in S] coef[0] (p_c - q_c) + [r valid] coef[1] (P1_c - [c = y]) ),
 *              exact zeros for the rows outside both sets and in columns [classes, ld), chosen by index.  Reads logits,
 *              teacher, labels, lse and coef as the forward left them.  rows == 0: nothing is launched.
 *   sigma_distill_loss_workspace_bytes    the bytes of `workspace` the forward needs (SIGMA_CE_BLOCKS slots of 4 floats), or
 *              -1 for parameters the launches refuse on their values (pointers are not looked at).
 *
 * SIGMA_OPS_ERR_ARG before any launch: NULL params; classes < 1 or > 64; ld or ld_t % 4 != 0 or < classes; rows < 0;
 * temperature not > 0, a negative kd_weight or ce_weight (NaN fails each); a missing pointer (logits, teacher, labels and
 * lse only when rows > 0); logits / teacher / dlogits off a 16-byte boundary, labels off 8, any other off 4; a workspace
 * smaller than the query's answer.
 */
#ifndef SIGMA_DISTILL_H_
#define SIGMA_DISTILL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sigma_distill_params {
    int64_t rows;
    int32_t classes, ld, ld_t;
    int32_t kd_all;                /* 0: S = the valid rows; otherwise S = every row                         */
    int64_t ignore_index;
    double temperature;            /* T                                                                      */
    double kd_weight, ce_weight;
    const float *logits;           /* (rows, ld): the student                                                */
    const float *teacher;          /* (rows, ld_t)                                                           */
    const int64_t *labels;         /* (rows)                                                                 */
    float *lse;                    /* (rows, 3): fwd out, bwd in                                             */
    void *workspace;               /* fwd scratch: sigma_distill_loss_workspace_bytes                        */
    int64_t workspace_bytes;
    float *loss;                   /* fwd out (1)                                                            */
    float *terms;                  /* fwd out (2): kd, mean cross entropy                                    */
    float *coef;                   /* (2): fwd out, bwd in                                                   */
    const float *scale;            /* bwd in (1): the upstream gradient G                                    */
    float *dlogits;                /* bwd out (rows, ld), every element written                              */
} sigma_distill_params;

int sigma_distill_loss_fwd(const sigma_distill_params *params, void *stream);
int sigma_distill_loss_bwd(const sigma_distill_params *params, void *stream);
int64_t sigma_distill_loss_workspace_bytes(const sigma_distill_params *params);

#ifdef __cplusplus
}
#endif

#endif /* SIGMA_DISTILL_H_ */
