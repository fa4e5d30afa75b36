// extern "C" entry points, part 9: the stage-major driver of ONE backbone stage over a whole sequence (SURVEY.md §8b:
// rvt_stage_seq_fwd), and the ONE place that decides a stage's kernel routes (rvt_stage_routes).  The no-grad forward — validation
// and streaming inference (reference modules/detection.py:231-255 calling maxvit_rnn.py:93-105,169-182 once per time step) — runs the
// host loop of rvt_amd/stage.py (workspace carving, block loop, the per-step ConvLSTM launches) here in C++: one C call per stage
// instead of 20-60 Python-level operator calls (the streaming step of RVT-Base, B = 64, was 4.1 ms of host enqueue for 0.9 ms of
// kernels).  The block loop and the scan tail are shared with the training driver (capi_train.hip).  Nothing is launched that the
// operator entry points do not launch; this file only sequences them.
#include <vector>
#include "host.hpp"

using namespace rvt;

namespace rvt {
int stage_blocks_fwd(const RvtStageDesc& d, const RvtStageRoutes& r, const StageShape& s, const void* inp, void* prepack, void* y0, void* x0,
                     const RvtBlockSaved* blk, void* stream) {
    const int C = d.C, F = s.F, H = s.H, W = s.W, M = s.M, dt = d.dtype;
    // ---- down-sampling conv + LayerNorm (maxvit.py:174-178) ----
    if (d.inp_u8 && rvt_stem_supported(dt, 1, d.Cin, C, d.k, d.stride, d.pad, d.w_raw)) {
        RVT_TRY(rvt_stem_fwd(inp, d.conv_w, d.ln_w, d.ln_b, y0, x0, dt, F, d.Cin, d.cin_pad, d.h_raw, d.w_raw, d.H_in, d.W_in, d.eps, stream));
    } else {
        if (d.inp_u8) {                                   // loader planes, no stem kernel for this shape: cast + pad + repack first
            RVT_CHECK(prepack != nullptr, "stage forward: uint8 planes need the stem kernels (the host prepacks otherwise)");
            RVT_TRY(rvt_prepack_input(inp, 1, prepack, dt, F, d.Cin, d.h_raw, d.w_raw, d.H_in, d.W_in, d.cin_pad, stream));
            inp = prepack;
        }
        RVT_TRY(rvt_conv_fwd(inp, d.conv_w, y0, dt, F, d.H_in, d.W_in, d.cin_pad, C, d.k, d.stride, d.pad, stream));
        RVT_TRY(rvt_layernorm_fwd(y0, d.ln_w, d.ln_b, x0, dt, M, C, d.eps, stream));
    }
    // ---- attention blocks (maxvit.py:267-270): window, then grid ----
    const void* x = x0;
    for (int bi = 0; bi < 2 * d.num_blocks; bi++) {
        const RvtBlockWeights& bw = d.blocks[bi];
        const RvtBlockSaved& b = blk[bi];
        const int window = (bi & 1) == 0;
        RVT_CHECK(b.xin == x && b.xmid != nullptr && b.xout != nullptr, "stage forward: block %d buffers inconsistent", bi);
        if (r.attn_block) {
            RVT_TRY(rvt_attn_block_fwd(x, b.xmid, b.a, bw.n1_w, bw.n1_b, bw.qkv_w, bw.qkv_b, bw.proj_w, bw.proj_b, bw.g1, dt, F, H, W, C,
                                       d.dim_head, d.ph, d.pw, window, d.eps, stream));
        } else {
            RVT_CHECK(b.qkv != nullptr && b.a != nullptr && (bw.n1_w == nullptr || r.ln_linear || b.u != nullptr), "stage forward: block %d misses qkv / a / u", bi);
            if (r.ln_linear) {
                RVT_TRY(rvt_ln_linear_fwd(x, bw.n1_w, bw.n1_b, bw.qkv_w, bw.qkv_b, bw.n1_w != nullptr ? b.u : nullptr, b.qkv, dt, M, C, 3 * C, d.eps, stream));
            } else {
                const void* uu = x;
                if (bw.n1_w != nullptr) { RVT_TRY(rvt_layernorm_fwd(x, bw.n1_w, bw.n1_b, b.u, dt, M, C, d.eps, stream)); uu = b.u; }
                RVT_TRY(rvt_linear_fwd(uu, bw.qkv_w, bw.qkv_b, b.qkv, dt, M, 3 * C, C, 0, stream));
            }
            RVT_TRY(rvt_attn_fwd(b.qkv, b.a, dt, F, H, W, C, d.dim_head, d.ph, d.pw, window, stream));
            RVT_TRY(rvt_linear_scale_res_fwd(b.a, bw.proj_w, bw.proj_b, bw.g1, x, b.xmid, dt, M, C, C, 0, stream));
        }
        if (r.mlp_route != 0) {
            RVT_TRY(rvt_mlp_fwd(b.xmid, b.xout, nullptr, nullptr, nullptr, bw.n2_w, bw.n2_b, bw.fc1_w, bw.fc1_b, bw.fc2_w, bw.fc2_b, bw.g2, dt, M, C,
                                d.eps, stream));
        } else {
            RVT_CHECK(b.v2 != nullptr && b.hg != nullptr, "stage forward: block %d misses v2 / hg", bi);
            RVT_TRY(rvt_layernorm_fwd(b.xmid, bw.n2_w, bw.n2_b, b.v2, dt, M, C, d.eps, stream));
            RVT_TRY(rvt_linear_gelu_fwd(b.v2, bw.fc1_w, bw.fc1_b, b.hg, b.hgp, dt, M, 4 * C, C, stream));
            RVT_TRY(rvt_linear_scale_res_fwd(b.hg, bw.fc2_w, bw.fc2_b, bw.g2, b.xmid, b.xout, dt, M, C, 4 * C, 0, stream));
        }
        x = b.xout;
    }
    return 0;
}

int stage_lstm_fwd(const RvtStageDesc& d, const RvtStageRoutes& r, const StageShape& s, const void* x, void* Hall, const float* c0,
                   float* c_last, void* Csave, void* gates, const void* wp3, const LstmStep* steps, int T, void* stream) {
    if (r.lstm_route == 3) {
        RVT_CHECK(wp3 != nullptr, "stage forward: lstm_scan3 weights missing");
        return rvt_lstm_scan3_fwd(x, Hall, c0, c_last, Csave, wp3, d.lstm_bn, gates, d.dtype, s.Ms, d.C, T, r.lstm_scan3_rb, stream);
    }
    if (r.lstm_route != 0)
        return rvt_lstm_scan_fwd(x, Hall, c0, c_last, Csave, d.lstm_wn, d.lstm_bn, r.lstm_route == 2 ? gates : nullptr, d.dtype, s.Ms, d.C, T, stream);
    for (int t = 0; t < T; t++) {
        const LstmStep& k = steps[t];
        RVT_TRY(rvt_lstm_fwd((const char*)x + (size_t)t * s.state * s.e, k.h_in, k.c_in, d.lstm_w, d.lstm_b, k.h_out, k.c_out, k.gates, d.dtype, s.Ms, d.C, stream));
    }
    return 0;
}
}  // namespace rvt

namespace {
// Every piece the no-grad driver takes from its workspace, in the order it takes them.  On a counting Carver this is
// rvt_stage_seq_fwd_ws_bytes: a piece the routes do not use is neither carved nor counted.
struct FwdCarve {
    void* bufs[3];                // activation ring: y0 / x / xmid / xout
    void* pk;                     // loader planes without a stem kernel for this shape are prepacked here
    RvtBlockSaved scratch;        // op-by-op halves: u, qkv, a / v2, GELU(h) - one set shared by all blocks
    float* cbuf[2];               // per-step ConvLSTM: cell-state ping-pong
    void* wp;                     // lstm_scan3: the weights in operand order
};
static FwdCarve carve_fwd(Carver& cv, const RvtStageDesc& d, const RvtStageRoutes& r, const StageShape& s) {
    FwdCarve c;
    memset(&c, 0, sizeof(c));
    for (void*& b : c.bufs) b = cv.take(s.act);
    if (d.inp_u8 && !rvt_stem_supported(d.dtype, 1, d.Cin, d.C, d.k, d.stride, d.pad, d.w_raw)) c.pk = cv.take((size_t)s.F * d.H_in * d.W_in * d.cin_pad * s.e);
    if (!r.attn_block) { c.scratch.u = r.ln_linear ? nullptr : cv.take(s.act); c.scratch.qkv = cv.take(3 * s.act); c.scratch.a = cv.take(s.act); }
    if (r.mlp_route == 0) { c.scratch.v2 = cv.take(s.act); c.scratch.hg = cv.take(4 * s.act); }
    if (r.lstm_route == 3) c.wp = cv.take((size_t)8 * d.C * d.C * s.e);
    else if (r.lstm_route == 0) for (float*& b : c.cbuf) b = (float*)cv.take(s.state * 4);
    return c;
}
static size_t fwd_ws_bytes(const RvtStageDesc& d, const RvtStageRoutes& r, const StageShape& s) {
    Carver cv = Carver::counting(256);
    carve_fwd(cv, d, r, s);
    return cv.bytes();
}
}  // namespace

extern "C" {

// ---- the routes of one stage: the only code that turns (tuning record, rvt_*_supported answers, shape) into stage-level routes ----
int rvt_stage_routes(const RvtStageDesc* dp, int T, int B, int save, int has_dws, int has_token_mask, RvtStageRoutes* out) {
    RVT_CHECK(dp != nullptr && out != nullptr && dp->struct_bytes == (int)sizeof(RvtStageDesc) && T >= 1 && B >= 1,
              "stage_routes: bad arguments (struct_bytes must be sizeof(RvtStageDesc) = %d)", (int)sizeof(RvtStageDesc));
    const RvtStageDesc& d = *dp;
    const RvtTuning& tn = tuning();
    const int dt = d.dtype, C = d.C, n_tok = d.ph * d.pw;
    StageShape s;
    stage_shape(d, T, B, nullptr, &s);
    const int Ms = s.Ms;                                   // tokens per time step
    RvtStageRoutes r;
    memset(&r, 0, sizeof(r));

    // Attention half of a block (norm1, qkv, partition attention, proj, LayerScale + residual) as ONE kernel per direction
    // (attn_block.hpp, one wave per partition) instead of LayerNorm + linear + attention core + linear (+ their backward chain): where
    // it is built (C = 64, dim_head 32, partitions of 33..96 tokens).  tuning.route_attn_block = 0 disables.  Partitions of more than
    // 64 tokens (Gen1: 8 x 10) have a fused forward only: a forward that keeps activations for a backward takes the op-by-op chain there.
    r.attn_block = !(save && n_tok > 64) && tn.route_attn_block != 0 && rvt_attn_block_supported(dt, C, d.dim_head, n_tok);
    // op-by-op attention: norm1 + qkv in one launch (ln_linear.hpp; C = 128), and in the backward the qkv / fc1 input gradient with
    // the LayerNorm backward behind it (dgrad_ln.hpp)
    r.ln_linear = !r.attn_block && rvt_ln_linear_supported(dt, C, 3 * C);
    r.dgrad_ln_qkv = rvt_linear_dgrad_ln_supported(dt, C, 3 * C) != 0;
    r.dgrad_ln_fc1 = rvt_linear_dgrad_ln_supported(dt, C, 4 * C) != 0;
    // the first block of a stage has no norm1 (maxvit_rnn.py:153 `skip_first_norm`): with nothing between it and the down-sampling
    // norm (no token mask), its backward launch carries the gradient through that norm too (dy0 instead of dx)
    r.attn_preln = (r.attn_block || r.dgrad_ln_qkv) && tn.route_attn_preln != 0 && !has_token_mask && d.num_blocks > 0 &&
                   d.blocks != nullptr && d.blocks[0].n1_w == nullptr;

    // Which MLP halves go through the fused kernels of mlp.hpp / mlp_chain.hpp.
    //   route 1 (C = 64): the whole backward — recompute of LN2 / fc1 / GELU, both input-gradient products, LayerNorm backward and the
    //       weight gradients (two launches, or ONE: mlp_bwd_both) — from (dxout, xmid) alone; the forward then saves nothing but the
    //       block input (3 + 2 rows of C per token through HBM for the MLP half instead of 32), and the no-grad forward takes the same
    //       kernel, so eval and training outputs are bit-identical.
    //   route 2 (C in {64, 128}): fused forward, saving GELU / GELU' / LN2 out for the backward (at C = 128 by default only the
    //       pre-activation h: mlp_store_pre; the backward applies GELU on load in the fc2 weight gradient and GELU' in the epilogue of
    //       the fc2 input gradient), and the fused input-gradient chain (mlp_bwd_dgrad).  Measured on MI355X
    //       (profiles/microbench_mlp.py, bf16, ms, fused vs op-by-op chain):
    //       C=64 : training forward 3.00 / 3.72, inference forward 2.03 / 3.72, backward dgrad chain 2.31 / 3.51 -> fused
    //       C=128: training forward 1.75 / 2.11, inference forward 1.53 / 2.11                                    -> fused
    //              backward dgrad chain 2.19 / 1.89 (one workgroup per CU: registers)                            -> chain
    //   A forward that keeps nothing launches the same rvt_mlp_fwd on either route: it is recorded as route 1.
    // tuning.route_fused_mlp = 1 forces every supported case (used by the parity tests), 0 disables all;
    // tuning.route_mlp_bwd_fused = 0 disables only the everything-on-chip backward.
    const int mlp_mode = tn.route_fused_mlp;
    const bool mlp_fused = mlp_mode != 0 && rvt_mlp_fused_supported(dt, C);
    if (mlp_mode != 0 && tn.route_mlp_bwd_fused != 0 && rvt_mlp_bwd_fused_supported(dt, C)) r.mlp_route = 1;
    else if (mlp_fused && (mlp_mode == 1 || C == 64 || C == 128)) r.mlp_route = save ? 2 : 1;
    r.mlp_bwd_both = r.mlp_route == 1 && rvt_mlp_bwd_both_supported(dt, C);
    r.mlp_bwd_dgrad = r.mlp_route == 2 && (mlp_mode == 1 || C == 64);
    r.mlp_store_pre = r.mlp_route == 2 && tn.route_mlp_store_pre != 0 && !r.mlp_bwd_dgrad;

    // ConvLSTM with the time loop inside the kernel instead of one launch per step: only the 1x1-conv cell (dws_conv False — every
    // shipped config).
    //   route 3 (lstm_scan3.hpp; bf16, C = 128 / 256): weights streamed from L2 in operand order, gates saved for the reverse scan:
    //       instead of 3 launches per step at C = 256 (weights too large for the chip), instead of route 2 at C = 128 — except below
    //       16384 tokens per step (stage 3 of RVT-Tiny), which stay on the register-resident weights of route 2.  Measured with both
    //       kernels in one process (profiles/scan_route2/microbench_parent.txt; T = 21, ms, route 3 at rb = 1 against route 2):
    //         tokens   forward + reverse scan            no-grad forward
    //            640   0.084 + 0.132 / 0.113 + 0.171     0.081 / 0.086
    //           2560   0.088 + 0.134 / 0.118 + 0.174     0.082 / 0.087
    //           7680   0.111 + 0.164 / 0.131 + 0.198     0.096 / 0.092
    //          92160   1.050 + 1.445 / 1.498 + 2.168     0.793 / 1.076
    //       Since the one-block-per-wave split route 2 no longer wins a training step anywhere; what it still wins is the no-grad
    //       forward at 7680 tokens, by 0.004 ms where its own timings spread 0.001.  That kept it from being retired, and the
    //       exception stands as it was until that point is settled.
    //   routes 1 / 2 (lstm_scan.hpp, lstm_scan2.hpp): by default where the weights stay resident in LDS (C <= 64; gates recomputed by
    //       the reverse scan, which can also accumulate the weight gradients: lstm_scan_wgrad) or in the register file (bf16 C = 128;
    //       gates saved: route 2); tuning.route_lstm_scan = 1: all supported widths (the parity tests); 0 disables.
    //   One no-grad step (streaming inference, T = 1) keeps the per-step GEMM: it beats staging the scan's weights (3.69 vs 3.81 ms per
    //   step at B = 64), and packing + streaming them buys nothing there.
    const int scan_mode = tn.route_lstm_scan;
    if (!has_dws && rvt_lstm_scan3_supported(dt, C) && !(C == 128 && Ms < 16384 && scan_mode != 0) && (save || T > 1)) {
        r.lstm_route = 3;
        // Forward tile: 64 tokens (rb = 2) stream half the weight bytes per token, but halve the tile count.  They are the default
        // where every workgroup the chip holds gets a 64-token tile: Ms / 64 >= 256 CUs x (256 / C) workgroups per CU, i.e.
        // Ms C >= 2^22 (C = 256: 16384 tokens, C = 128: 32768).  Forward, T = 21, 64- against 32-token tiles (parent: its best):
        //   C = 256, 23040 tokens (360 tiles): 0.765 against 1.000 ms (0.950);   C = 128, 92160 (1440): 0.948 against 1.220 (1.235);
        //   C = 256, 640 (stage 4 of RVT-Tiny: 10 tiles on 256 CUs): 0.284 against 0.214 (0.215);   C = 128, 2560: 0.132 against 0.085.
        // The tuning record still forces 64 (lstm_scan3_rb128 / _rb256 = 2: the tests and the microbenchmark).
        r.lstm_scan3_rb = rvt_lstm_scan3_rb(C) == 2 || (long long)Ms * C >= (1ll << 22) ? 2 : 1;
    } else if (!has_dws && scan_mode != 0 && rvt_lstm_scan_supported(dt, C) && !(scan_mode == -1 && T == 1 && !save) &&
               (scan_mode == 1 || C <= 64 || rvt_lstm_scan_saves_gates(dt, C))) {
        r.lstm_route = rvt_lstm_scan_saves_gates(dt, C) ? 2 : 1;
    }
    r.lstm_scan_wgrad = r.lstm_route == 1 && tn.route_lstm_scan_wgrad != 0 && rvt_lstm_scan_bwd_ws_floats(dt, C, Ms) > 0;
    r.conv_dgrad4 = tn.route_conv_dgrad4 != 0 && rvt_conv_dgrad4_supported(dt, d.H_in, d.W_in, d.Cin, C, d.k, d.stride, d.pad, T * B);
    // what the C-side drivers sequence; the training driver also leaves the saving fused-MLP flavour to the host loop
    r.driver_covers = !has_dws && !has_token_mask && (!save || r.mlp_route != 2);
    *out = r;
    return 0;
}

size_t rvt_stage_seq_fwd_ws_bytes(const RvtStageDesc* d, int T, int B) {
    RvtStageRoutes r;
    StageShape s;
    if (rvt_stage_routes(d, T, B, 0, 0, 0, &r) != 0 || stage_shape(*d, T, B, nullptr, &s) != 0) return 0;
    return fwd_ws_bytes(*d, r, s);
}

int rvt_stage_seq_fwd(const RvtStageDesc* dp, const void* inp, const void* h0, const float* c0, void* Hall, float* c_last,
                      void* ws, size_t ws_bytes, int T, int B, void* stream) {
    RvtStageRoutes r;
    RVT_TRY(rvt_stage_routes(dp, T, B, 0, 0, 0, &r));
    const RvtStageDesc& d = *dp;
    RVT_CHECK(d.num_blocks >= 0 && d.blocks != nullptr && inp != nullptr && Hall != nullptr && c_last != nullptr, "stage_seq_fwd: bad arguments");
    RVT_CHECK((h0 == nullptr) == (c0 == nullptr), "stage_seq_fwd: h0 and c0 go together");
    StageShape s;
    RVT_TRY(stage_shape(d, T, B, "stage_seq_fwd", &s));
    const size_t need = fwd_ws_bytes(d, r, s);
    RVT_CHECK(ws != nullptr && ws_bytes >= need, "stage_seq_fwd: workspace of %zu bytes < rvt_stage_seq_fwd_ws_bytes = %zu", ws_bytes, need);
    Carver cv{(char*)ws, ws_bytes, 256};
    const FwdCarve c = carve_fwd(cv, d, r, s);
    RVT_CHECK(cv.ok, "stage_seq_fwd: workspace carving overflow");
    hipStream_t st = (hipStream_t)stream;

    // the block table of a forward that keeps nothing: three ping-pong activations, one scratch set shared by all blocks
    std::vector<RvtBlockSaved> blk(2 * d.num_blocks, c.scratch);
    int xi = 1;                                           // bufs[xi] = the running activation
    for (RvtBlockSaved& b : blk) {
        const int mi = (xi + 1) % 3, oi = 3 - xi - mi;
        b.xin = c.bufs[xi]; b.xmid = c.bufs[mi]; b.xout = c.bufs[oi];
        xi = oi;
    }
    RVT_TRY(stage_blocks_fwd(d, r, s, inp, c.pk, c.bufs[0], c.bufs[1], blk.data(), stream));

    // ---- ConvLSTM over the T steps (rnn.py:43-67); Hall slot 0 = incoming h, slots 1..T = the stage's output features ----
    char* const HallB = (char*)Hall;
    const size_t hB = s.state * s.e;                      // bytes of one h slot
    // None state -> zeros (rnn.py:43-47); the scan kernels want the incoming h in slot 0, the per-step route reads it where it is
    if (h0 == nullptr) RVT_HIP(hipMemsetAsync(HallB, 0, hB, st), "stage_seq_fwd: memset");
    else if (r.lstm_route != 0) RVT_HIP(hipMemcpyAsync(HallB, h0, hB, hipMemcpyDeviceToDevice, st), "stage_seq_fwd: state copy");
    if (c.wp != nullptr) RVT_TRY(rvt_lstm_scan3_pack(d.lstm_wn, c.wp, nullptr, d.C, stream));
    std::vector<LstmStep> steps;
    if (r.lstm_route == 0) {                              // c ping-pongs between two buffers; the last step writes c_last
        const void* h_prev = h0 != nullptr ? h0 : HallB;
        const float* c_prev = c0;
        if (c0 == nullptr) { RVT_HIP(hipMemsetAsync(c.cbuf[1], 0, s.state * 4, st), "stage_seq_fwd: memset"); c_prev = c.cbuf[1]; }
        for (int t = 0; t < T; t++) {
            steps.push_back(LstmStep{h_prev, c_prev, HallB + (size_t)(t + 1) * hB, t + 1 == T ? c_last : c.cbuf[t & 1], nullptr});
            h_prev = steps[t].h_out; c_prev = steps[t].c_out;
        }
    }
    RVT_TRY(stage_lstm_fwd(d, r, s, c.bufs[xi], Hall, c0, c_last, nullptr, nullptr, c.wp, steps.data(), T, stream));
    return check_launch("stage_seq_fwd");
}

}  // extern "C"
