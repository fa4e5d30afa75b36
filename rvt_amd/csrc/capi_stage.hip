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
int stage_blocks_fwd(const RvtStageDesc& d, const RvtStageRoutes& r, const void* inp, void* prepack, void* y0, void* x0,
                     const RvtBlockSaved* blk, int T, int B, void* stream) {
    const int C = d.C, F = T * B, dt = d.dtype;
    const int H = conv_out(d.H_in, d.k, d.stride, d.pad), W = conv_out(d.W_in, d.k, d.stride, d.pad), M = F * H * W;
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

int stage_lstm_scan_fwd(const RvtStageDesc& d, const RvtStageRoutes& r, const void* x, void* Hall, const float* c0, float* c_last,
                        void* Csave, void* gates, const void* wp3, int T, int B, void* stream) {
    const int Ms = B * conv_out(d.H_in, d.k, d.stride, d.pad) * conv_out(d.W_in, d.k, d.stride, d.pad);
    if (r.lstm_route == 3) {
        RVT_CHECK(wp3 != nullptr, "stage forward: lstm_scan3 weights missing");
        return rvt_lstm_scan3_fwd(x, Hall, c0, c_last, Csave, wp3, d.lstm_bn, gates, d.dtype, Ms, d.C, T, r.lstm_scan3_rb, stream);
    }
    return rvt_lstm_scan_fwd(x, Hall, c0, c_last, Csave, d.lstm_wn, d.lstm_bn, r.lstm_route == 2 ? gates : nullptr, d.dtype, Ms, d.C, T, stream);
}
}  // namespace rvt

namespace {
static size_t stage_ws_bytes(const RvtStageDesc& d, const RvtStageRoutes& r, int T, int B) {
    const int H = conv_out(d.H_in, d.k, d.stride, d.pad), W = conv_out(d.W_in, d.k, d.stride, d.pad);
    const size_t tok = (size_t)T * B * H * W, e = elt_bytes(d.dtype), pad = 256;
    size_t n = 3 * (tok * d.C * e + pad);                                   // activation ping-pong (y0 / x / xmid / xout)
    if (!r.attn_block) n += tok * d.C * e * 5 + 3 * pad;                    // u, qkv (3C), a
    if (r.mlp_route == 0) n += tok * d.C * e * 5 + 2 * pad;                 // v2, GELU(h) (4C)
    if (!d.inp_u8 || !rvt_stem_supported(d.dtype, 1, d.Cin, d.C, d.k, d.stride, d.pad, d.w_raw))
        n += d.inp_u8 ? (size_t)T * B * d.H_in * d.W_in * d.cin_pad * e + pad : 0;      // prepacked input
    n += 2 * ((size_t)B * H * W * d.C * 4 + pad);                           // cell-state ping-pong of the per-step route
    n += (size_t)8 * d.C * d.C * e + pad;                                   // ConvLSTM weights in operand order (lstm_scan3 route)
    return n + 4096;
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
    const int Ms = B * conv_out(d.H_in, d.k, d.stride, d.pad) * conv_out(d.W_in, d.k, d.stride, d.pad);     // tokens per time step
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
    if (rvt_stage_routes(d, T, B, 0, 0, 0, &r) != 0) return 0;
    return stage_ws_bytes(*d, r, T, B);
}

int rvt_stage_seq_fwd(const RvtStageDesc* dp, const void* inp, const void* h0, const float* c0, void* Hall, float* c_last,
                      void* ws, size_t ws_bytes, int T, int B, void* stream) {
    RvtStageRoutes r;
    RVT_TRY(rvt_stage_routes(dp, T, B, 0, 0, 0, &r));
    const RvtStageDesc& d = *dp;
    RVT_CHECK(d.num_blocks >= 0 && d.blocks != nullptr && inp != nullptr && Hall != nullptr && c_last != nullptr, "stage_seq_fwd: bad arguments");
    RVT_CHECK((h0 == nullptr) == (c0 == nullptr), "stage_seq_fwd: h0 and c0 go together");
    RVT_CHECK(ws != nullptr && ws_bytes >= stage_ws_bytes(d, r, T, B), "stage_seq_fwd: workspace of %zu bytes < rvt_stage_seq_fwd_ws_bytes = %zu",
              ws_bytes, stage_ws_bytes(d, r, T, B));
    const int C = d.C, F = T * B, dt = d.dtype;
    const int H = conv_out(d.H_in, d.k, d.stride, d.pad), W = conv_out(d.W_in, d.k, d.stride, d.pad);
    RVT_CHECK(H % d.ph == 0 && W % d.pw == 0, "stage_seq_fwd: %dx%d not divisible by the partition %dx%d", H, W, d.ph, d.pw);
    const size_t e = elt_bytes(dt), tok = (size_t)F * H * W, act = tok * C * e;
    RVT_CHECK(tok * 4 * C < ((size_t)1 << 31), "stage_seq_fwd: %zu token rows exceed the operators' 32-bit sizes", tok);
    Carver cv{(char*)ws, ws_bytes, 256};
    void* bufs[3] = {cv.take(act), cv.take(act), cv.take(act)};
    hipStream_t st = (hipStream_t)stream;
    void* pk = nullptr;                                   // loader planes without a stem kernel for this shape are prepacked here
    if (d.inp_u8 && !rvt_stem_supported(dt, 1, d.Cin, C, d.k, d.stride, d.pad, d.w_raw)) pk = cv.take((size_t)F * d.H_in * d.W_in * d.cin_pad * e);

    // the block table of a forward that keeps nothing: three ping-pong activations, one scratch set shared by all blocks
    RvtBlockSaved scratch;
    memset(&scratch, 0, sizeof(scratch));
    if (!r.attn_block) { scratch.u = r.ln_linear ? nullptr : cv.take(act); scratch.qkv = cv.take(3 * act); scratch.a = cv.take(act); }
    if (r.mlp_route == 0) { scratch.v2 = cv.take(act); scratch.hg = cv.take(4 * act); }
    RVT_CHECK(cv.ok, "stage_seq_fwd: workspace carving overflow");
    std::vector<RvtBlockSaved> blk(2 * d.num_blocks, scratch);
    int xi = 1;                                           // bufs[xi] = the running activation
    for (RvtBlockSaved& b : blk) {
        const int mi = (xi + 1) % 3, oi = 3 - xi - mi;
        b.xin = bufs[xi]; b.xmid = bufs[mi]; b.xout = bufs[oi];
        xi = oi;
    }
    RVT_TRY(stage_blocks_fwd(d, r, inp, pk, bufs[0], bufs[1], blk.data(), T, B, stream));
    const void* x = bufs[xi];

    // ---- ConvLSTM over the T steps (rnn.py:43-67); Hall slot 0 = incoming h, slots 1..T = the stage's output features ----
    const size_t sN = (size_t)B * H * W * C;             // elements of one state
    const int Ms = B * H * W;
    char* const HallB = (char*)Hall;
    if (r.lstm_route != 0) {
        void* wp = r.lstm_route == 3 ? cv.take((size_t)8 * C * C * e) : nullptr;
        RVT_CHECK(cv.ok, "stage_seq_fwd: workspace carving overflow");
        if (h0 != nullptr) { if (hipMemcpyAsync(HallB, h0, sN * e, hipMemcpyDeviceToDevice, st) != hipSuccess) { set_last_error("stage_seq_fwd: state copy failed"); return 1; } }
        else if (hipMemsetAsync(HallB, 0, sN * e, st) != hipSuccess) { set_last_error("stage_seq_fwd: memset failed"); return 1; }
        if (wp != nullptr) RVT_TRY(rvt_lstm_scan3_pack(d.lstm_wn, wp, nullptr, C, stream));
        RVT_TRY(stage_lstm_scan_fwd(d, r, x, Hall, c0, c_last, nullptr, nullptr, wp, T, B, stream));
    } else {
        float* cbuf[2] = {(float*)cv.take(sN * 4), (float*)cv.take(sN * 4)};
        RVT_CHECK(cv.ok, "stage_seq_fwd: workspace carving overflow");
        const void* h_prev = h0;
        const float* c_prev = c0;
        if (h0 == nullptr) {                              // None state -> zeros (rnn.py:43-47)
            if (hipMemsetAsync(HallB, 0, sN * e, st) != hipSuccess || hipMemsetAsync(cbuf[1], 0, sN * 4, st) != hipSuccess) {
                set_last_error("stage_seq_fwd: memset failed"); return 1;
            }
            h_prev = HallB; c_prev = cbuf[1];
        }
        for (int t = 0; t < T; t++) {
            float* c_out = t + 1 == T ? c_last : cbuf[t & 1];
            RVT_TRY(rvt_lstm_fwd((const char*)x + (size_t)t * sN * e, h_prev, c_prev, d.lstm_w, d.lstm_b, HallB + (size_t)(t + 1) * sN * e, c_out,
                                 nullptr, dt, Ms, C, stream));
            h_prev = HallB + (size_t)(t + 1) * sN * e;
            c_prev = c_out;
        }
    }
    return check_launch("stage_seq_fwd");
}

}  // extern "C"
