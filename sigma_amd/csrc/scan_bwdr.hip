// scan_bwdr.hip -- selective-scan backward, "row-lane" mapping (gfx950 / MI355X, wave64, f32 IO, ckpt_pitch 16).
//
// Same operator as scan_bwd4.hip (reference: models/encoders/selective_scan/csrc/selective_scan/
// selective_scan_bwd_kernel.cuh:66-308, reverse_scan.cuh:18-401; mathematics SURVEY.md App. E.2); the mapping is the one
// of scan_fwdr.hip (scan_rowlane.h): a lane is a channel row, a wave is 64 rows x NS states, B / C are SGPR operands,
// tiles of 16 positions, the state entering a tile comes from the forward's per-tile checkpoint.  Per element-state:
//     forward replay   v_mul, v_exp, v_mul, v_fma                                   (a, x kept for the tile: 32 registers)
//     reverse          v_fma (dx = g C + e), v_mul (e = a dx), v_fma (sum dx B), v_mul (t = e x_prev),
//                      v_fma (sum A t), v_fma (dA), v_mul (dx delta u), v_mul (g x)
// = 11 plain VALU + 1 v_exp, against 17.5 + 1.1 of the quad-row kernel's mathematics plus its mapping overhead (row
// scans, broadcasts, slabs, column sums; profiles/r03_bwd4_issue_model.md: 1170 clocks per 640 element-states).  What
// this mapping pays instead: the dB / dC terms of a (state, position) are spread over the 64 LANES of a wave.  They are
// summed by a transpose-reduce network per state and tile: 32 registers (16 positions x {dB, dC}) -> 1 register in which
// every lane pair holds the total of one slot: 24 lane swaps (v_permlane32_swap, v_permlane16_swap) + 24 adds + 15 DPP
// adds + 1 select, ~20 clocks per 64 element-states.  The totals of a row block leave through the per-block slabs of the caller's
// workspace (reduce_partials_kernel adds the blocks of a group in a fixed order: deterministic).
//
// Few rows: the sequence is cut into S segments; rev_summary (MODE 1 of the same body) writes per segment, row and state
// (decay product P, reverse value E from zero), a segment composes the summaries to its right into its incoming carry.
#include "scan_device.h"
#include "scan_launch.h"
#include "scan_rowlane.h"

#include <type_traits>

// The one build switch of the kernels: a wait that keeps SIGMA_BWDR_WAIT_SKEW vector-memory operations too many in flight.
// It exists only for the negative case of tests/test_isa_waits_cpu.py, which compiles a mis-counted build to prove that its
// ISA check refuses one.  The product build leaves it at 0.
#ifndef SIGMA_BWDR_WAIT_SKEW
#define SIGMA_BWDR_WAIT_SKEW 0
#endif

namespace sigma {

namespace {

// Sum of the dB / dC terms of a tile over the 64 lanes.  The 32 slots of a tile are (memory half hm, position j in the
// half, array dB / dC).  rl_reduce_half takes the eight fold32(dB term, dC term) registers of ONE half (w[j]: lanes 0-31
// = dB of position j summed over lane pairs l, l + 32; lanes 32-63 = dC) to ONE register in which every lane holds the sum
// over 16 lanes of one slot; rl_reduce_finish merges the registers of the two halves: on return lane l holds the total of
//     array  l >> 5,   memory position  8 * bit1(l) + 2 * bit2(l) + bit3(l) + 4 * bit4(l)       (each total in lanes l, l ^ 1).
// Stages: halves of the wave (permlane32_swap: runs as soon as a position is done), row pairs (permlane16_swap: positions
// j and j + 4), inside a DPP row distance 8 and 4 by DPP adds under bank masks (a disabled lane keeps what the other add
// of the pair wrote), distance 2 by two quad permutes + one select, distance 1 by a quad permute.  The network was
// checked lane by lane with a symbolic model (tools/rowlane_reduce_model.py prints the table above).
// Hazard: a VALU write followed by a DPP read of the same VGPR needs two wait states.
__device__ __forceinline__ float rl_reduce_half(const float (&w)[8]) {
    const float z0 = fold16(w[0], w[4]), z1 = fold16(w[1], w[5]), z2 = fold16(w[2], w[6]), z3 = fold16(w[3], w[7]);
    float q0, q1, ph;
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %3, %3 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %1, %5, %5 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %0, %4, %4 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %1, %6, %6 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %2, %0, %0 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %2, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
        : "=&v"(q0), "=&v"(q1), "=&v"(ph)
        : "v"(z0), "v"(z1), "v"(z2), "v"(z3));
    return ph;
}

// p0 = rl_reduce_half of memory half 0, p1 = of memory half 1
__device__ __forceinline__ float rl_reduce_finish(float p0, float p1) {
    float t0, t1, o;
    const unsigned long long lanes_bit1 = 0xCCCCCCCCCCCCCCCCull;
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %3, %3 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %4, %4 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32 %2, %0, %1, %5\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        : "=&v"(t0), "=&v"(t1), "=&v"(o)
        : "v"(p0), "v"(p1), "s"(lanes_bit1));
    return o;
}

// 16 bytes of a row; `ok` false: zeros (the load itself always runs, from the row start, so that the VMEM operations of a
// tile are the same on every path and the compiler's vmcnt bookkeeping stays exact instead of falling back to vmcnt(0))
__device__ __forceinline__ v4f rl_load4u(const float* __restrict__ row, int off, bool ok) {
    const v4f z = {0.0f, 0.0f, 0.0f, 0.0f};
    const v4f t = *reinterpret_cast<const v4f*>(row + (ok ? off : 0));
    return ok ? t : z;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// The backward proper.  A workgroup is one block of 64 rows x 4 state waves (NS = dstate / 4 states each).  Per tile of 16
// positions: the (row, chunk) threads pre-process u / delta / dout once (softplus, delta * u, softplus') into LDS; then
// every wave runs, for each of its states: forward replay of the tile from the forward's checkpoint (one per tile,
// scan_rowlane.h), the reverse recurrence, the sums over the states of dx B and A2 dx a x_prev in 16 registers, and the
// lane-reduce of the dB / dC terms.
// One piece of work: scan steps [st_lo, st_hi) of one row block (sequence segment seg), walked from the last to the
// first.  The reverse carry entering at st_hi is zero (cin 0: no segments) or the composition of the summaries of the
// segments after this one (cin 1).
struct RlPiece { int b, g, rbg, st_lo, st_hi, cin, seg; };

template <int NS, bool REV, bool DET = false>
__device__ __forceinline__ void scan_bwdr_body(const BwdArgs& q, float* smem, const RlPiece pc) {
    constexpr int T = kRT, H = kRT / 2;
    // wave-uniform by construction (block index arithmetic); said explicitly, because integer divisions are expanded on
    // the vector ALU and would otherwise make every address derived from them look divergent (no scalar loads)
    const int b = __builtin_amdgcn_readfirstlane(pc.b), g = __builtin_amdgcn_readfirstlane(pc.g);
    const int rbg = __builtin_amdgcn_readfirstlane(pc.rbg), seg = __builtin_amdgcn_readfirstlane(pc.seg);
    const FwdArgs& p = q.f;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int sw = __builtin_amdgcn_readfirstlane(tid >> 6);      // state wave 0..3
    const int N = p.N, L = p.L;
    const int ntiles = (L + T - 1) / T;
    v4f* sProc = reinterpret_cast<v4f*>(smem);                    // [5][4][64] float4: delta, delta * u, dout; u, softplus' (epilogue)
    v4f* sEx = sProc + 5 * 256;                                   // [4 waves][2][4][64] float4: sum dx B, sum A2 dx a x_prev
    v4f* sRaw = sEx + 8 * 256;                                    // [3][256 threads] float4: u, delta, dout of the NEXT tile (LDS-DMA)
    const unsigned raw_base = (unsigned)(uintptr_t)(lptr_t)(sRaw + sw * 64);   // this wave's 1 KB of array 0

    // thread as (row, chunk)
    const int rr = (sw << 4) | (lane >> 2), cc = lane & 3;
    const int rpg = p.rows_per_group;
    const int row0 = g * rpg + rbg * kRRows;
    const int r_rc = row0 + rr;
    const int ur_rc = r_rc - ((g - (g >> p.u_gshift)) * rpg);     // same row of group g >> u_gshift
    const int gr_rc = r_rc - ((g - (g >> q.g_gshift)) * rpg);
    // rows of this thread as wave-uniform bases (the block's first row; SGPRs) + 32-bit element offsets (the row inside
    // the block and the chunk): five 64-bit per-thread pointers less across the state loops (host: 64 rows x stride < 2^29)
    const int ur0 = row0 - ((g - (g >> p.u_gshift)) * rpg), gr0 = row0 - ((g - (g >> q.g_gshift)) * rpg);
    const float* u_blk = reinterpret_cast<const float*>(p.u) + (long)b * p.u_bs + (long)ur0 * p.u_ds;
    const float* d_blk = reinterpret_cast<const float*>(p.delta) + (long)b * p.dt_bs + (long)row0 * p.dt_ds;
    const float* g_blk = reinterpret_cast<const float*>(q.dout) + (long)b * q.g_bs + (long)gr0 * q.g_ds;
    float* du_blk = reinterpret_cast<float*>(q.du) + (long)b * q.du_bs + (long)row0 * q.du_ds;
    float* dd_blk = reinterpret_cast<float*>(q.ddelta) + (long)b * q.dd_bs + (long)row0 * q.dd_ds;
    const int u_off = rr * (int)p.u_ds + 4 * cc, d_off = rr * (int)p.dt_ds + 4 * cc, g_off = rr * (int)q.g_ds + 4 * cc;
    const int du_off = rr * (int)q.du_ds + 4 * cc, dd_off = rr * (int)q.dd_ds + 4 * cc;
    (void)ur_rc; (void)gr_rc;
    const int pr_rc = param_row(r_rc, g, rpg, p.pswap);
    const float bias = p.bias ? p.bias[pr_rc] : 0.0f;
    const float Dd = p.D ? p.D[pr_rc] : 0.0f;
    float dD_acc = 0.0f, dbias_acc = 0.0f;

    // thread as row lane
    const int pr_ln = param_row(row0 + lane, g, rpg, p.pswap);
    const int n0 = sw * NS;
    float A2[NS], ecar[NS], dAacc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        A2[s] = p.A[(long)pr_ln * p.A_ds + (long)(n0 + s) * p.A_ns] * kLog2e;
        ecar[s] = 0.0f;
        dAacc[s] = 0.0f;
    }
    const float* Bw = reinterpret_cast<const float*>(p.B) + (long)b * p.B_bs + (long)g * p.B_gs + (long)n0 * p.B_ns;
    const float* Cw = reinterpret_cast<const float*>(p.C) + (long)b * p.C_bs + (long)g * p.C_gs + (long)n0 * p.C_ns;
    const int B_ns = (int)p.B_ns, C_ns = (int)p.C_ns;               // host: (N - 1) * stride + L fits 31 bits
    const long rowblock = (long)b * (p.dim >> 6) + (row0 >> 6);
    // checkpoints (one per tile): x[(rowblock * ntiles + tile) * N * 64 + rl_ck_slot(n, lane)] = state after memory tile `tile` in scan order
    const float* ck = p.x + rowblock * ntiles * N * 64;                         // wave-uniform; rl_load_ck adds the wave's slot

    // dB / dC of this row block: the caller's tensors when the block is the whole group, else its slab of the workspace
    float* __restrict__ oB;
    float* __restrict__ oC;
    long o_nsB, o_nsC;
    if (q.P == 1) {
        oB = q.dB + (long)b * q.dB_bs + (long)g * q.dB_gs; o_nsB = q.dB_ns;
        oC = q.dC + (long)b * q.dC_bs + (long)g * q.dC_gs; o_nsC = q.dC_ns;
    } else {
        const long slab = (((long)rbg * p.batch + b) * p.G + g) * (long)N * L;
        oB = q.ws_dB + slab; oC = q.ws_dC + slab; o_nsB = L; o_nsC = L;
    }
    // lane l of rl_reduce_finish: array l >> 5, memory position below (lanes l and l ^ 1 hold the same total and store it twice)
    const int o_pos = ((lane >> 1) & 1) * 8 + ((lane >> 2) & 1) * 2 + ((lane >> 3) & 1) + ((lane >> 4) & 1) * 4;
    float* __restrict__ o_lane = (lane < 32 ? oB + (long)n0 * o_nsB : oC + (long)n0 * o_nsC) + o_pos;
    const int o_ns_lane = (int)(lane < 32 ? o_nsB : o_nsC);

    // scan steps [st_lo, st_hi) of this workgroup, walked from the last to the first
    const int st_lo = __builtin_amdgcn_readfirstlane(pc.st_lo), st_hi = __builtin_amdgcn_readfirstlane(pc.st_hi);
    const int nst = st_hi - st_lo;
    if (pc.cin) {
        // reverse carry entering the right end = composition of the summaries of the segments after this one
        const float2* __restrict__ sm = reinterpret_cast<const float2*>(q.summ);
        // eight summaries requested at once (as in the forward: one iteration per segment waited for its own loads)
        const long sm_seg = (long)p.batch * (p.dim >> 6) * N * 64;
        const float2* __restrict__ sm0 = sm + ((long)rowblock * N + n0) * 64 + lane;
        int t = q.S - 1;
        for (; t - 8 >= seg; t -= 8) {
            float2 pe[8][NS];
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int s = 0; s < NS; ++s) pe[k][s] = sm0[(long)(t - 1 - k) * sm_seg + s * 64];
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int s = 0; s < NS; ++s) ecar[s] = fmaf(pe[k][s].x, ecar[s], pe[k][s].y);
        }
        for (; t > seg; --t) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float2 pe = sm0[(long)(t - 1) * sm_seg + s * 64];
                ecar[s] = fmaf(pe.x, ecar[s], pe.y);
            }
        }
    }
    auto tile_of = [&](int st) { return REV ? (ntiles - 1 - st) : st; };   // memory tile of scan step st
    // u / delta / dout of a tile travel by LDS-DMA one tile ahead (with register targets the compiler, short of
    // registers, moved the requests next to their use: three exposed memory latencies per tile).  Chunks past the end of
    // the row are requested at the row start (memory the row owns) and replaced by selects when they are read back: the
    // row start may hold NaN or inf, and 0 * that is NaN.
    auto request = [&](int mt) {
        const int tl = T * mt + 4 * cc < L ? T * mt : -4 * cc;      // past the end: the row start
        rl_dma16s(u_blk, (unsigned)(u_off + tl) * 4u, raw_base);
        rl_dma16s(d_blk, (unsigned)(d_off + tl) * 4u, raw_base + 256 * 16);
        rl_dma16s(g_blk, (unsigned)(g_off + tl) * 4u, raw_base + 512 * 16);
    };
    int st = st_hi - 1;
    int m = tile_of(st);
    request(m);
    float x1_nx[NS];                                                // the states entering the next step
    // the NS states entering scan step st_ = those after the previous step's tile: one access per lane (before the first
    // step there is none: the load is clamped to a valid block and the value replaced by zero where it is used -- by a
    // select, the block may hold a non-finite state; a select next to the load would make the compiler wait for it there)
    auto ck_load = [&](int st_, float (&xo)[NS]) {
        rl_load_ck<NS, NS>(ck + (unsigned)(tile_of(st_ > 0 ? st_ - 1 : 0) * N * 64), n0, lane, xo);      // host: floats per row block < 2^31
    };
    ck_load(st, x1_nx);
    // B / C of the NEXT tile are pulled into L2 a tile ahead (see scan_fwdr.hip)
    const float* __restrict__ bc_touch = ((lane & 1) ? Cw : Bw) + (long)((lane >> 1) & (NS - 1)) * ((lane & 1) ? C_ns : B_ns);
    float touch_nx = 0.0f, touch_acc = 0.0f;

    auto step = [&](int it, auto tail_tag) {
        constexpr bool TAIL = decltype(tail_tag)::value;
        st = st_hi - 1 - it;
        m = tile_of(st);
        const bool valid = !TAIL || T * m + 4 * cc < L;
        const int nch = TAIL ? (L - T * m) >> 2 : 4;                // valid 16-byte chunks of this tile
        float Bn[T], Cn[T];
        rl_load_bc(Bw + T * m, nch, Bn);                            // first state's B / C: requested before anything waits
        rl_load_bc(Cw + T * m, nch, Cn);
        __builtin_amdgcn_sched_barrier(0);
        // This tile's u / delta / dout have landed.  A full step of the loop issues 4 + NS vector-memory operations
        // after its requests (the touch, ONE checkpoint load, NS dB/dC stores, du, ddelta), which stay in
        // flight; the partial tile may skip some of them, so it (and the step after it: the caller waits) drains the counter.
        if (TAIL) rl_dma_wait(); else rl_dma_wait_keep<4 + NS + SIGMA_BWDR_WAIT_SKEW>();
        v4f uu = sRaw[tid];
        const v4f dd = sRaw[256 + tid];
        v4f g4 = sRaw[512 + tid];
        const v4f zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
        g4 = valid ? g4 : zero4;                                    // dout and u read as zero past the end
        uu = valid ? uu : zero4;
        float x1[NS];
        touch_acc += touch_nx;
#pragma unroll
        for (int s = 0; s < NS; ++s) x1[s] = x1_nx[s];                                   // x1: the state entering this tile
        {                                                           // next tile's operands fly during this tile
            const bool more = it + 1 < nst;
            const int mn = tile_of(more ? st - 1 : st);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the reads of this tile's bytes are done
            request(mn);
            touch_nx = bc_touch[T * mn];
        }
        {
            v4f dl4, dlu4, sg4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float raw = dd[j] + bias;
                float sig;
                const float sp = softplus_ref(raw, sig);
                float d = p.softplus ? sp : raw;
                sg4[j] = p.softplus ? sig : 1.0f;
                d = valid ? d : 0.0f;                               // identity element past the end (a = 1, b = 0)
                dl4[j] = d;
                dlu4[j] = d * uu[j];
                dD_acc = fmaf(g4[j], uu[j], dD_acc);
            }
            // the epilogue of this tile reads its operands back (they would cost 16 registers across the state loops)
            sProc[rl_unit(cc, rr)] = dl4;
            sProc[256 + rl_unit(cc, rr)] = dlu4;
            sProc[512 + rl_unit(cc, rr)] = g4;
            sProc[768 + rl_unit(cc, rr)] = uu;
            sProc[1024 + rl_unit(cc, rr)] = sg4;
        }
        lds_barrier();

        {
            float dl[T], dlu[T], gg[T], sdxB[T], sAx[T];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const v4f a4 = sProc[rl_unit(c, lane)], b4 = sProc[256 + rl_unit(c, lane)], g4r = sProc[512 + rl_unit(c, lane)];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    dl[4 * c + j] = a4[j]; dlu[4 * c + j] = b4[j]; gg[4 * c + j] = g4r[j];
                    sdxB[4 * c + j] = 0.0f; sAx[4 * c + j] = 0.0f;
                }
            }
            // LDS reads and scalar loads share one counter: retire the reads before the first scalar request of the state loop
            asm volatile("" : "+v"(dl[0]), "+v"(dlu[0]), "+v"(gg[0]), "+v"(dl[4]), "+v"(dlu[4]), "+v"(gg[4]),
                              "+v"(dl[8]), "+v"(dlu[8]), "+v"(gg[8]), "+v"(dl[12]), "+v"(dlu[12]), "+v"(gg[12]));
            __builtin_amdgcn_sched_barrier(0);
            const bool has_xin = st > 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float Bt[T], Ct[T];
#pragma unroll
                for (int k = 0; k < T; ++k) { Bt[k] = Bn[k]; Ct[k] = Cn[k]; }
                // scalar loads return out of order: wait for THIS state's operands (lgkmcnt(0)), then request the next state's
                asm volatile("" : "+s"(Bt[0]), "+s"(Ct[0]));
                __builtin_amdgcn_sched_barrier(0);
                if (s + 1 < NS) {
                    rl_load_bc(Bw + (s + 1) * B_ns + T * m, nch, Bn);
                    rl_load_bc(Cw + (s + 1) * C_ns + T * m, nch, Cn);
                }
                __builtin_amdgcn_sched_barrier(0);
                const float xin = has_xin ? x1[s] : 0.0f;
                float a[T], xs[T];
                // ---- forward replay of the tile from the state entering it
                {
                    float x = xin;
#pragma unroll
                    for (int kk = 0; kk < T; ++kk) {
                        const int k = REV ? T - 1 - kk : kk;
                        // past the end (partial tile only; wave-uniform): the identity step, whatever A, B and x hold
                        const bool live = !TAIL || T * m + k < L;
                        a[k] = live ? fast_exp2(dl[k] * A2[s]) : 1.0f;
                        x = live ? fmaf(a[k], x, dlu[k] * Bt[k]) : x;
                        xs[k] = x;
                    }
                }
                // ---- reverse: dx_k = g_k C_k + e_{k+1}, e_k = a_k dx_k
                float e = ecar[s];
                float w[H], ph_first = 0.0f;
#pragma unroll
                for (int kk = T - 1; kk >= 0; --kk) {
                    const int k = REV ? T - 1 - kk : kk;
                    const bool live = !TAIL || T * m + k < L;
                    const float dx = live ? fmaf(gg[k], Ct[k], e) : e;
                    e = a[k] * dx;
                    const int kp = REV ? k + 1 : k - 1;             // previous position in scan order
                    const float xprev = kk > 0 ? xs[kk > 0 ? kp : k] : xin;
                    sdxB[k] = fmaf(dx, Bt[k], sdxB[k]);
                    const float t = live ? e * xprev : 0.0f;        // dx * a_k * x_{k-1}
                    sAx[k] = fmaf(A2[s], t, sAx[k]);                // x ln 2 in the epilogue
                    dAacc[s] = fmaf(dl[k], t, dAacc[s]);
                    w[k & 7] = fold32(dx * dlu[k], gg[k] * xs[k]);  // this row's terms of dB[n, l] and dC[n, l], wave halves summed
                    if (kk == H) {                                  // the half walked first is complete: memory half REV ? 0 : 1
                        ph_first = rl_reduce_half(w);
                    }
                }
                ecar[s] = e;
                const float ph_second = rl_reduce_half(w);          // memory half REV ? 1 : 0
                const float tot = REV ? rl_reduce_finish(ph_first, ph_second) : rl_reduce_finish(ph_second, ph_first);
                if (!TAIL || T * m + o_pos < L) o_lane[s * o_ns_lane + T * m] = tot;
                __builtin_amdgcn_sched_barrier(0);
            }
            // ---- the sums over the states of the four waves meet in LDS
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const v4f t1 = {sdxB[4 * c], sdxB[4 * c + 1], sdxB[4 * c + 2], sdxB[4 * c + 3]};
                const v4f t2 = {sAx[4 * c], sAx[4 * c + 1], sAx[4 * c + 2], sAx[4 * c + 3]};
                sEx[(sw * 2) * 256 + rl_unit(c, lane)] = t1;
                sEx[(sw * 2 + 1) * 256 + rl_unit(c, lane)] = t2;
            }
            ck_load(it + 1 < nst ? st - 1 : st, x1_nx);              // the states entering the NEXT step
        }
        lds_barrier();
        {
            v4f S1 = {0.0f, 0.0f, 0.0f, 0.0f}, S2 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int w = 0; w < 4; ++w) { S1 += sEx[(w * 2) * 256 + rl_unit(cc, rr)]; S2 += sEx[(w * 2 + 1) * 256 + rl_unit(cc, rr)]; }
            const v4f dle = sProc[rl_unit(cc, rr)], ge = sProc[512 + rl_unit(cc, rr)];
            const v4f ue = sProc[768 + rl_unit(cc, rr)], sge = sProc[1024 + rl_unit(cc, rr)];
            v4f duv, ddv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                duv[j] = fmaf(Dd, ge[j], dle[j] * S1[j]);
                ddv[j] = fmaf(ue[j], S1[j], S2[j] * kLn2) * sge[j];
                dbias_acc += valid ? ddv[j] : 0.0f;
            }
            if (valid) {
                *reinterpret_cast<v4f*>(du_blk + (unsigned)(du_off + T * m)) = duv;
                *reinterpret_cast<v4f*>(dd_blk + (unsigned)(dd_off + T * m)) = ddv;
            }
        }
    };
    // The partial tile (fewer than 16 positions: the memory-last one) is the first step of a forward group and the last
    // of a reversed one: it is peeled off the loop.  With both variants of the body inside ONE loop the register
    // allocation of the whole loop doubled (254 instead of 128 VGPRs at 16 states).
    const int tail_tile = (L % T) ? ntiles - 1 : -1;                // memory tile with fewer than 16 positions
    int it0 = 0, it1 = nst;
    rl_dma_wait();                                                  // the first requests: nothing younger behind them yet
    if (!REV && nst > 0 && tile_of(st_hi - 1) == tail_tile) {
        step(0, std::true_type{});
        it0 = 1;
        rl_dma_wait();
    }
    if (REV && nst > 0 && tile_of(st_lo) == tail_tile) it1 = nst - 1;
    for (int it = it0; it < it1; ++it) step(it, std::false_type{});
    if (it1 < nst) step(it1, std::true_type{});
    if (touch_acc == 1.2345678e-30f) du_blk[0] = touch_acc;        // keeps the touches alive (never true in practice)

    // per-row results: one atomicAdd per (row, state) / row and workgroup (several workgroups only with segments);
    // deterministic mode (MODE 3): one store each into slot b * S + seg of the row partials
    const int rk = b * q.S + seg;
#pragma unroll
    for (int s = 0; s < NS; ++s) row_result<DET>(&q, q.dA + (long)pr_ln * q.dA_ds + (long)(n0 + s) * q.dA_ns, rk, pr_ln, n0 + s, true, dAacc[s]);
    // the four chunk threads of a row are neighbouring lanes
    dD_acc += dpp_take<0xB1, 0xF>(0.0f, dD_acc);                    // quad_perm [1,0,3,2]
    dD_acc += dpp_take<0x4E, 0xF>(0.0f, dD_acc);                    // quad_perm [2,3,0,1]
    dbias_acc += dpp_take<0xB1, 0xF>(0.0f, dbias_acc);
    dbias_acc += dpp_take<0x4E, 0xF>(0.0f, dbias_acc);
    if (cc == 0) {
        if (q.dD) row_result<DET>(&q, q.dD + pr_rc, rk, pr_rc, N, true, dD_acc);
        if (q.dbias) row_result<DET>(&q, q.dbias + pr_rc, rk, pr_rc, N + 1, true, dbias_acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Reverse summaries of the sequence split: for segment seg = 1 .. S-1, row and state the pair (decay product P, reverse
// value E with zero carry): e(left end of the segment) = E + P * e(right end).  The reverse recurrence only.
template <int NS, bool REV>
__device__ __forceinline__ void scan_bwdr_summary_body(const BwdArgs& q, float* smem, int b, int g, int rbg, int seg) {
    constexpr int T = kRT;
    const FwdArgs& p = q.f;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int sw = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = p.N, L = p.L;
    const int ntiles = (L + T - 1) / T;
    v4f* sProc = reinterpret_cast<v4f*>(smem);                    // [2][4][64] float4: delta, dout
    const int rr = (sw << 4) | (lane >> 2), cc = lane & 3;
    const int rpg = p.rows_per_group;
    const int row0 = g * rpg + rbg * kRRows;
    const int r_rc = row0 + rr;
    const int gr_rc = r_rc - ((g - (g >> q.g_gshift)) * rpg);
    const float* __restrict__ d_row = reinterpret_cast<const float*>(p.delta) + (long)b * p.dt_bs + (long)r_rc * p.dt_ds;
    const float* __restrict__ g_row = reinterpret_cast<const float*>(q.dout) + (long)b * q.g_bs + (long)gr_rc * q.g_ds;
    const int pr_rc = param_row(r_rc, g, rpg, p.pswap);
    const float bias = p.bias ? p.bias[pr_rc] : 0.0f;
    const int pr_ln = param_row(row0 + lane, g, rpg, p.pswap);
    const int n0 = sw * NS;
    float A2[NS], ecar[NS], Pacc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        A2[s] = p.A[(long)pr_ln * p.A_ds + (long)(n0 + s) * p.A_ns] * kLog2e;
        ecar[s] = 0.0f;
        Pacc[s] = 0.0f;                                             // log2 of the decay product
    }
    const float* Cw = reinterpret_cast<const float*>(p.C) + (long)b * p.C_bs + (long)g * p.C_gs + (long)n0 * p.C_ns;
    const int C_ns = (int)p.C_ns;
    const long rowblock = (long)b * (p.dim >> 6) + (row0 >> 6);
    const int st_lo = seg * q.seg_tiles;
    const int st_hi = st_lo + q.seg_tiles < ntiles ? st_lo + q.seg_tiles : ntiles;
    const int nst = st_hi - st_lo;
    auto tile_of = [&](int st) { return REV ? (ntiles - 1 - st) : st; };
    int m = tile_of(st_hi - 1);
    v4f d_nx = rl_load4u(d_row, T * m + 4 * cc, T * m + 4 * cc < L);
    v4f g_nx = rl_load4u(g_row, T * m + 4 * cc, T * m + 4 * cc < L);
    for (int it = 0; it < nst; ++it) {
        const int st = st_hi - 1 - it;
        m = tile_of(st);
        const bool valid = T * m + 4 * cc < L;
        const v4f dd = d_nx, g4 = g_nx;
        {
            const bool more = it + 1 < nst;
            const int mn = tile_of(more ? st - 1 : st);
            d_nx = rl_load4u(d_row, T * mn + 4 * cc, more && T * mn + 4 * cc < L);
            g_nx = rl_load4u(g_row, T * mn + 4 * cc, more && T * mn + 4 * cc < L);
        }
        const int nch = (L - T * m) >= T ? 4 : (L - T * m) >> 2;
        v4f dl4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float raw = dd[j] + bias;
            float sig;
            const float sp = softplus_ref(raw, sig);
            const float d = p.softplus ? sp : raw;
            dl4[j] = valid ? d : 0.0f;
        }
        sProc[rl_unit(cc, rr)] = dl4;
        sProc[256 + rl_unit(cc, rr)] = g4;
        lds_barrier();
        float dl[T], gg[T];
        float dsum = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const v4f a4 = sProc[rl_unit(c, lane)], g4r = sProc[256 + rl_unit(c, lane)];
#pragma unroll
            for (int j = 0; j < 4; ++j) { dl[4 * c + j] = a4[j]; gg[4 * c + j] = g4r[j]; dsum += a4[j]; }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float Ct[T];
            rl_load_bc(Cw + s * C_ns + T * m, nch, Ct);
            float e = ecar[s];
#pragma unroll
            for (int kk = T - 1; kk >= 0; --kk) {
                const int k = REV ? T - 1 - kk : kk;
                e = fast_exp2(dl[k] * A2[s]) * fmaf(gg[k], Ct[k], e);
            }
            ecar[s] = e;
            Pacc[s] = fmaf(dsum, A2[s], Pacc[s]);
        }
        lds_barrier();
    }
    float2* __restrict__ sm = reinterpret_cast<float2*>(q.summ);
#pragma unroll
    for (int s = 0; s < NS; ++s)
        sm[(((long)(seg - 1) * p.batch * (p.dim >> 6) + rowblock) * N + n0 + s) * 64 + lane] = make_float2(fast_exp2(Pacc[s]), ecar[s]);
}

// MODE 0: the backward proper; MODE 1: the summaries of segments 1 .. S-1; MODE 3: the backward proper in deterministic
// mode (per-row results stored to the slots of q.rpart, no atomics).  MODE 2 is retired (a single-kernel chained walk:
// measured, no gain, removed -- profiles/r04_rowlane_chain.txt); the numbers stay, kernel traces name these symbols.
// Waves per SIMD the register allocation is sized for: the 64 KB of LDS of the backward proper (bwdr_lds_bytes) admit two
// workgroups per CU = 2 waves per SIMD = 256 VGPRs; asking for 3 (round 4) capped the 16-state build at 168 VGPRs with 81
// spilled to scratch for an occupancy the LDS never allowed.
template <int NS, int MODE>
__global__ void __launch_bounds__(256, MODE == 1 ? 4 : 2)
scan_bwdr_kernel(const BwdArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    static_assert(MODE == 0 || MODE == 1 || MODE == 3, "MODE 2 is retired");
    const int ntiles = (q.f.L + kRT - 1) / kRT;
    const int lb = xcd_logical_block(blockIdx.x, gridDim.x);
    const int S = MODE == 1 ? q.S - 1 : q.S;
    const int PS = q.P * S;                                   // workgroups per (batch, group): row blocks x segments
    const int per_b = q.f.G * PS;
    const int b = __builtin_amdgcn_readfirstlane(lb / per_b);
    const int rem = lb - b * per_b;
    const int g = __builtin_amdgcn_readfirstlane(rem / PS);
    const int rem2 = rem - g * PS;
    const int rbg = __builtin_amdgcn_readfirstlane(rem2 / S);
    const int seg = rem2 - rbg * S + (MODE == 1 ? 1 : 0);
    const bool rev = (q.f.rev_mask >> g) & 1u;
    if (MODE == 1) {
        if (rev) scan_bwdr_summary_body<NS, true>(q, smem, b, g, rbg, seg);
        else scan_bwdr_summary_body<NS, false>(q, smem, b, g, rbg, seg);
    } else {
        RlPiece pc;
        pc.b = b; pc.g = g; pc.rbg = rbg; pc.seg = seg;
        pc.st_lo = q.S > 1 ? seg * q.seg_tiles : 0;
        pc.st_hi = q.S > 1 ? (pc.st_lo + q.seg_tiles < ntiles ? pc.st_lo + q.seg_tiles : ntiles) : ntiles;
        pc.cin = q.S > 1 ? 1 : 0;
        if (rev) scan_bwdr_body<NS, true, MODE == 3>(q, smem, pc);
        else scan_bwdr_body<NS, false, MODE == 3>(q, smem, pc);
    }
}

template <int NS, int MODE>
static hipError_t launch_bwdr_t(const BwdArgs& a, hipStream_t stream) {
    const int S = MODE == 1 ? a.S - 1 : a.S;
    const int grid = (int)((long)a.f.batch * a.f.G * a.P * S);       // one workgroup per (row block, segment)
    const size_t lds = bwdr_lds_bytes(4);
    constexpr auto kern = scan_bwdr_kernel<NS, MODE>;
    if (hipError_t e = raise_lds_cap<kern>(lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, a);
    return hipGetLastError();
}

template <int MODE>
static hipError_t launch_bwdr_ns(const BwdArgs& a, hipStream_t stream) {
    switch (a.f.N) {
        case 16: return launch_bwdr_t<4, MODE>(a, stream);
        case 8: return launch_bwdr_t<2, MODE>(a, stream);
        case 4: return launch_bwdr_t<1, MODE>(a, stream);
        default: return hipErrorInvalidValue;
    }
}

// a.P = 64-row blocks per (batch, group); a.S segments of a.seg_tiles tiles (a.summ when S > 1)
hipError_t launch_scan_bwdr(const BwdArgs& a, hipStream_t stream) {
    hipError_t e;
    if (a.S > 1) {
        e = launch_bwdr_ns<1>(a, stream);
        if (e != hipSuccess) return e;
    }
    e = a.rpart ? launch_bwdr_ns<3>(a, stream) : launch_bwdr_ns<0>(a, stream);
    if (e != hipSuccess) return e;
    return launch_reduce_after(a, stream);
}

}  // namespace sigma
