// extern "C" entry points, part 11: the TRAINING-side stage driver (rvt_stage_seq_bwd; round 6) — the training
// forward and the BPTT backward of one backbone stage (reference maxvit_rnn.py:169-182 under autograd, over the loop of
// modules/detection.py:131-148) as one call each.  The launch sequences are the ones rvt_amd/stage.py (stage_seq_forward with
// save=True / stage_seq_backward) issues from Python, in the same order, with the same arguments: outputs are bit-identical
// (tests/test_stage_driver.py).  The routes come from rvt_stage_routes (capi_stage.hip), copied by the host into RvtStageTrain when
// the forward is planned and read back unchanged by the backward; the host owns everything that outlives a call (saved activations,
// gradient buckets); this file owns the order of launches and the backward's temporaries.  The forward's block loop and scan tail are
// the ones of the no-grad driver (host.hpp: stage_blocks_fwd, stage_lstm_fwd).  Nothing is launched that the operator entry
// points do not launch.
#include <vector>
#include "host.hpp"

using namespace rvt;

namespace {
static inline size_t zmax(size_t a, size_t b) { return a > b ? a : b; }

// what the backward's operators ask for as fp32 workspace on these routes (0 = that operator does not run)
struct BwdFloats { size_t wgrad, mlp, scan, stem; };
static BwdFloats bwd_floats(const RvtStageDesc& d, const RvtStageRoutes& r, const StageShape& s) {
    const int C = d.C, M = s.M;
    size_t w = rvt_wgrad_workspace_floats(d.dtype, 4 * C, 2 * C, M, 1);
    w = zmax(w, rvt_wgrad_workspace_floats(d.dtype, C, 4 * C, M, 1));
    w = zmax(w, rvt_wgrad_workspace_floats(d.dtype, 4 * C, C, M, 1));
    w = zmax(w, rvt_wgrad_workspace_floats(d.dtype, C, C, M, 1));
    w = zmax(w, rvt_wgrad_workspace_floats(d.dtype, 3 * C, C, M, 1));
    w = zmax(w, rvt_wgrad_workspace_floats(d.dtype, C, d.k * d.k * d.cin_pad, M, 0));
    BwdFloats f;
    f.wgrad = zmax(w, (size_t)1 << 20);
    f.mlp = r.mlp_route == 1 ? rvt_mlp_bwd_fused_ws_floats(d.dtype, C, M) : 0;
    f.scan = (r.lstm_route == 1 && r.lstm_scan_wgrad) ? rvt_lstm_scan_bwd_ws_floats(d.dtype, C, s.Ms) : 0;
    f.stem = d.inp_u8 ? rvt_stem_wgrad_ws_floats(d.Cin, s.F, d.H_in, d.W_in) : 0;
    return f;
}
// Every piece the backward takes from its workspace, in the order it takes them (a braced list is evaluated left to right).  On a
// counting Carver this is rvt_stage_seq_bwd_ws_bytes.
struct BwdCarve {
    void* ring[3];                // dx ring (block cotangents), [M][C] each
    void* big4;                   // [M][4C]: dz of the ConvLSTM, then dh of the op-by-op MLP
    void *dqkv, *t1, *dy0;        // [M][3C]; [M][C]: da / du / dv2; [M][C]
    void* dh_b;                   // one h state - per-step route: second dh buffer
    float *ws_wgrad, *ws_mlp, *ws_scan, *ws_stem;      // BwdFloats; NULL where 0
};
static BwdCarve carve_bwd(Carver& cv, const StageShape& s, const BwdFloats& f) {
    auto floats = [&cv](size_t n) { return n ? (float*)cv.take(n * 4) : nullptr; };
    return BwdCarve{{cv.take(s.act), cv.take(s.act), cv.take(s.act)}, cv.take(4 * s.act), cv.take(3 * s.act), cv.take(s.act), cv.take(s.act),
                    cv.take(s.state * s.e), floats(f.wgrad), floats(f.mlp), floats(f.scan), floats(f.stem)};
}
static size_t bwd_ws_bytes(const StageShape& s, const BwdFloats& f) {
    Carver cv = Carver::counting((size_t)1 << 21);
    carve_bwd(cv, s, f);
    return cv.bytes();
}
static bool desc_ok(const RvtStageDesc* d, const RvtStageTrain* t) {
    return d != nullptr && t != nullptr && d->struct_bytes == (int)sizeof(RvtStageDesc) && t->struct_bytes == (int)sizeof(RvtStageTrain) &&
           d->blocks != nullptr && t->saved != nullptr && d->num_blocks >= 0;
}
}  // namespace

extern "C" {

int rvt_stage_seq_train_fwd(const RvtStageDesc* dp, const RvtStageTrain* tp, const void* inp, const float* c0, int T, int B, void* stream) {
    RVT_CHECK(desc_ok(dp, tp), "stage_seq_train_fwd: bad descriptors (struct_bytes %d / %d expected)", (int)sizeof(RvtStageDesc), (int)sizeof(RvtStageTrain));
    const RvtStageDesc& d = *dp; const RvtStageTrain& t = *tp;
    RVT_CHECK(T >= 1 && B >= 1 && inp != nullptr && t.Hall != nullptr && t.c_last != nullptr && t.y0 != nullptr && t.x0 != nullptr,
              "stage_seq_train_fwd: bad arguments");
    StageShape s;
    RVT_TRY(stage_shape(d, T, B, "stage_seq_train_fwd", &s));
    const RvtStageRoutes& r = t.routes;
    const int nb = 2 * d.num_blocks;
    RVT_CHECK(r.driver_covers && (nb == 0 || t.saved[0].xin == t.x0), "stage_seq_train_fwd: routes the driver does not cover, or saved[0].xin != x0");
    for (int bi = 0; bi < nb; bi++)       // what the backward reads beyond what the forward itself needs
        RVT_CHECK(t.saved[bi].a != nullptr && (r.mlp_route != 0 || t.saved[bi].hgp != nullptr), "stage_seq_train_fwd: block %d misses a / hgp", bi);
    RVT_TRY(stage_blocks_fwd(d, r, s, inp, nullptr, t.y0, t.x0, t.saved, stream));
    const void* x = nb > 0 ? t.saved[nb - 1].xout : t.x0;
    // ---- ConvLSTM over the T steps (rnn.py:43-67); Hall slot 0 = incoming h, Call slot 0 = incoming c (host) ----
    std::vector<LstmStep> steps;
    if (r.lstm_route != 0) {
        RVT_CHECK(t.Csave != nullptr && (r.lstm_route == 1 || t.gates != nullptr), "stage_seq_train_fwd: scan buffers missing");
    } else {
        RVT_CHECK(t.Call != nullptr && t.gates != nullptr, "stage_seq_train_fwd: per-step ConvLSTM buffers missing");
        char* const HallB = (char*)t.Hall;
        const size_t hB = s.state * s.e;                  // bytes of one h slot
        for (int ts = 0; ts < T; ts++)                    // step ts: slot ts -> slot ts + 1 of Hall / Call, gates kept for BPTT
            steps.push_back(LstmStep{HallB + ts * hB, t.Call + ts * s.state, HallB + (ts + 1) * hB, t.Call + (ts + 1) * s.state, (char*)t.gates + ts * 4 * hB});
    }
    RVT_TRY(stage_lstm_fwd(d, r, s, x, t.Hall, c0, t.c_last, t.Csave, t.gates, t.lstm_wp3, steps.data(), T, stream));
    if (r.lstm_route == 0)
        RVT_HIP(hipMemcpyAsync(t.c_last, t.Call + (size_t)T * s.state, s.state * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream), "stage_seq_train_fwd: state copy");
    return check_launch("stage_seq_train_fwd");
}

size_t rvt_stage_seq_bwd_ws_bytes(const RvtStageDesc* d, const RvtStageTrain* t, int T, int B) {
    StageShape s;
    if (!desc_ok(d, t) || T < 1 || B < 1 || stage_shape(*d, T, B, nullptr, &s) != 0) return 0;
    return bwd_ws_bytes(s, bwd_floats(*d, t->routes, s));
}

int rvt_stage_seq_bwd(const RvtStageDesc* dp, const RvtStageTrain* tp, const void* inp, const void* dH, const float* dc_last,
                      const void* prev_cot, void* d_in, void* dh0, float* dc0, void* ws, size_t ws_bytes, int T, int B, void* stream) {
    RVT_CHECK(desc_ok(dp, tp) && tp->tb != nullptr, "stage_seq_bwd: bad descriptors");
    const RvtStageDesc& d = *dp; const RvtStageTrain& t = *tp;
    RVT_CHECK(T >= 1 && B >= 1 && inp != nullptr && dh0 != nullptr && dc0 != nullptr, "stage_seq_bwd: bad arguments");
    const RvtStageRoutes& r = t.routes;
    StageShape s;
    RVT_TRY(stage_shape(d, T, B, "stage_seq_bwd", &s));
    const BwdFloats f = bwd_floats(d, r, s);
    const size_t need = bwd_ws_bytes(s, f);
    RVT_CHECK(ws != nullptr && ws_bytes >= need, "stage_seq_bwd: workspace of %zu bytes < rvt_stage_seq_bwd_ws_bytes = %zu", ws_bytes, need);
    const int C = d.C, F = s.F, dt = d.dtype, H = s.H, W = s.W, M = s.M, Ms = s.Ms;
    hipStream_t st = (hipStream_t)stream;
    Carver cv{(char*)ws, ws_bytes, (size_t)1 << 21};
    const auto [ring, big4, dqkv, t1, dy0, dh_b, ws_wgrad, ws_mlp, ws_scan, ws_stem] = carve_bwd(cv, s, f);
    RVT_CHECK(cv.ok, "stage_seq_bwd: workspace carving overflow");
    const int nb = 2 * d.num_blocks;
    const void* x_last = nb > 0 ? t.saved[nb - 1].xout : t.x0;       // the ConvLSTM's input frames
    const char* const HallB = (const char*)t.Hall;

    // ---- ConvLSTM BPTT ----
    void* dx = ring[0];
    void* dz = big4;
    bool lstm_wgrad_done = false;
    if (r.lstm_route == 3) {
        RVT_TRY(rvt_lstm_scan3_bwd(t.gates, t.Csave, t.c0_saved, dH, dc_last, t.lstm_wtp3, dx, dz, dh0, dc0, dt, Ms, C, T, r.lstm_scan3_rb, stream));
    } else if (r.lstm_route == 1 || r.lstm_route == 2) {
        lstm_wgrad_done = r.lstm_route == 1 && r.lstm_scan_wgrad != 0;
        RVT_TRY(rvt_lstm_scan_bwd(x_last, t.Hall, t.Csave, t.c0_saved, dH, dc_last, d.lstm_wn, t.lstm_wt, d.lstm_bn, dx, lstm_wgrad_done ? nullptr : dz,
                                  dh0, dc0, lstm_wgrad_done ? t.d_lstm_w : nullptr, lstm_wgrad_done ? t.d_lstm_b : nullptr, ws_scan,
                                  r.lstm_route == 2 ? t.gates : nullptr, dt, Ms, C, T, stream));
    } else {
        RVT_CHECK(dH != nullptr, "stage_seq_bwd: the per-step route needs dH (zeros, not NULL)");
        if (dc_last != nullptr) RVT_HIP(hipMemcpyAsync(dc0, dc_last, s.state * 4, hipMemcpyDeviceToDevice, st), "stage_seq_bwd: copy");
        else RVT_HIP(hipMemsetAsync(dc0, 0, s.state * 4, st), "stage_seq_bwd: memset");
        void* dh_buf[2] = {dh0, dh_b};                   // step t writes dh_buf[t & 1]: the last one (t = 0) lands in dh0
        const void* dh_rec = nullptr;
        for (int ts = T - 1; ts >= 0; ts--) {
            char* const dz_t = (char*)dz + (size_t)ts * s.state * 4 * s.e;
            RVT_TRY(rvt_lstm_gates_bwd((const char*)dH + (size_t)ts * s.state * s.e, dh_rec, dc0, (const char*)t.gates + (size_t)ts * s.state * 4 * s.e,
                                       t.Call + (size_t)(ts + 1) * s.state, t.Call + (size_t)ts * s.state, dz_t, dt, Ms, C, stream));
            void* nxt = dh_buf[ts & 1];
            RVT_TRY(rvt_lstm_dgrad(dz_t, t.lstm_wt, (char*)dx + (size_t)ts * s.state * s.e, nxt, dt, Ms, C, stream));
            dh_rec = nxt;
        }
    }
    if (!lstm_wgrad_done)
        RVT_TRY(rvt_lstm_wgrad(dz, x_last, HallB, t.d_lstm_w, t.d_lstm_b, ws_wgrad, dt, M, C, stream));

    // ---- attention blocks, reversed ----
    bool preln_done = false;                                 // the first block's launch already wrote dy0 (rvt_attn_block_bwd_preln)
    int ri = 0;                                              // ring[ri] = the cotangent of the current block's output
    for (int bi = nb - 1; bi >= 0; bi--) {
        const RvtBlockWeights& bw = d.blocks[bi];
        const RvtBlockSaved& sv = t.saved[bi];
        const RvtBlockTrain& tb = t.tb[bi];
        const int window = (bi & 1) == 0;
        void* const dxo = ring[ri];
        void* const dxmid = ring[(ri + 1) % 3];
        void* const dxi = ring[(ri + 2) % 3];
        // MLP branch: xout = xmid + g2 * (gelu(h) W2^T + b2)
        if (r.mlp_route == 1) {
            if (r.mlp_bwd_both) {
                RVT_TRY(rvt_mlp_bwd_recompute_both(dxo, sv.xmid, dxmid, bw.n2_w, bw.n2_b, bw.fc1_w, bw.fc1_b, tb.fc2_wt, tb.fc1_wt, tb.d_n2_w, tb.d_n2_b,
                                                   tb.d_fc1_w, tb.d_fc1_b, tb.d_S2, tb.d_cs2, ws_mlp, dt, M, C, d.eps, stream));
            } else {
                RVT_TRY(rvt_mlp_bwd_recompute_wgrad(dxo, sv.xmid, bw.n2_w, bw.n2_b, bw.fc1_w, bw.fc1_b, tb.fc2_wt, tb.d_fc1_w, tb.d_fc1_b, tb.d_S2, tb.d_cs2,
                                                    ws_mlp, dt, M, C, d.eps, stream));
                RVT_TRY(rvt_mlp_bwd_recompute_dgrad(dxo, sv.xmid, dxmid, bw.n2_w, bw.n2_b, bw.fc1_w, bw.fc1_b, tb.fc2_wt, tb.fc1_wt, tb.d_n2_w, tb.d_n2_b,
                                                    dt, M, C, d.eps, stream));
            }
        } else {
            void* const dhd = big4;                          // (dz is consumed: rvt_lstm_wgrad is enqueued ahead on this stream)
            RVT_TRY(rvt_linear_wgrad(dxo, sv.hg, tb.d_S2, tb.d_cs2, ws_wgrad, dt, M, C, 4 * C, 0, stream));
            RVT_TRY(rvt_linear_dgrad(dxo, tb.fc2_wt, nullptr, nullptr, sv.hgp, dhd, dt, M, C, 4 * C, stream));
            RVT_TRY(rvt_linear_wgrad(dhd, sv.v2, tb.d_fc1_w, tb.d_fc1_b, ws_wgrad, dt, M, 4 * C, C, 0, stream));
            if (r.dgrad_ln_fc1) {
                RVT_TRY(rvt_linear_dgrad_ln(dhd, bw.fc1_w, sv.xmid, dxo, dxmid, bw.n2_w, tb.d_n2_w, tb.d_n2_b, dt, M, C, 4 * C, d.eps, stream));
            } else {
                RVT_TRY(rvt_linear_dgrad(dhd, tb.fc1_wt, nullptr, nullptr, nullptr, t1, dt, M, 4 * C, C, stream));
                RVT_TRY(rvt_layernorm_bwd(sv.xmid, bw.n2_w, t1, dxo, dxmid, tb.d_n2_w, tb.d_n2_b, dt, M, C, d.eps, stream));
            }
        }
        // attention branch: xmid = xin + g1 * (a Wp^T + bp)
        RVT_TRY(rvt_linear_wgrad(dxmid, sv.a, tb.d_S1, tb.d_cs1, ws_wgrad, dt, M, C, C, 0, stream));
        if (r.attn_block) {
            void* const u_out = bw.n1_w != nullptr ? t1 : nullptr;
            if (r.attn_preln && bi == 0 && bw.n1_w == nullptr) {
                // the stage's first block: the same launch carries the gradient through the down-sampling norm in front of it
                RVT_TRY(rvt_attn_block_bwd_preln(sv.xin, t.y0, dxmid, dy0, dqkv, d.ln_w, bw.qkv_w, bw.qkv_b, tb.proj_wt, t.d_ln_w, t.d_ln_b, dt, F, H, W,
                                                 C, d.dim_head, d.ph, d.pw, window, d.eps, stream));
                preln_done = true;
            } else {
                RVT_TRY(rvt_attn_block_bwd(sv.xin, dxmid, dxi, dqkv, u_out, bw.n1_w, bw.n1_b, bw.qkv_w, bw.qkv_b, tb.proj_wt, tb.d_n1_w, tb.d_n1_b, dt, F, H, W,
                                           C, d.dim_head, d.ph, d.pw, window, d.eps, stream));
            }
            RVT_TRY(rvt_linear_wgrad(dqkv, u_out != nullptr ? u_out : sv.xin, tb.d_qkv_w, tb.d_qkv_b, ws_wgrad, dt, M, 3 * C, C, 0, stream));
        } else {
            RVT_TRY(rvt_linear_dgrad(dxmid, tb.proj_wt, nullptr, nullptr, nullptr, t1, dt, M, C, C, stream));          // da
            RVT_TRY(rvt_attn_bwd(sv.qkv, t1, dqkv, dt, F, H, W, C, d.dim_head, d.ph, d.pw, window, stream));
            RVT_TRY(rvt_linear_wgrad(dqkv, bw.n1_w != nullptr ? sv.u : sv.xin, tb.d_qkv_w, tb.d_qkv_b, ws_wgrad, dt, M, 3 * C, C, 0, stream));
            if (bw.n1_w == nullptr && bi == 0 && r.attn_preln) {
                // the stage's first block: qkv input gradient + residual cotangent carried through the down-sampling norm (one launch)
                RVT_TRY(rvt_linear_dgrad_preln(dqkv, bw.qkv_w, t.y0, dxmid, dy0, d.ln_w, t.d_ln_w, t.d_ln_b, dt, M, C, 3 * C, d.eps, stream));
                preln_done = true;
            } else if (bw.n1_w == nullptr) {
                RVT_TRY(rvt_linear_dgrad(dqkv, tb.qkv_wt, nullptr, dxmid, nullptr, dxi, dt, M, 3 * C, C, stream));
            } else if (r.dgrad_ln_qkv) {
                RVT_TRY(rvt_linear_dgrad_ln(dqkv, bw.qkv_w, sv.xin, dxmid, dxi, bw.n1_w, tb.d_n1_w, tb.d_n1_b, dt, M, C, 3 * C, d.eps, stream));
            } else {
                RVT_TRY(rvt_linear_dgrad(dqkv, tb.qkv_wt, nullptr, nullptr, nullptr, t1, dt, M, 3 * C, C, stream));   // du
                RVT_TRY(rvt_layernorm_bwd(sv.xin, bw.n1_w, t1, dxmid, dxi, tb.d_n1_w, tb.d_n1_b, dt, M, C, d.eps, stream));
            }
        }
        ri = (ri + 2) % 3;
    }
    // ---- down-sampling LayerNorm + conv ----
    if (!preln_done) RVT_TRY(rvt_layernorm_bwd(t.y0, d.ln_w, ring[ri], nullptr, dy0, t.d_ln_w, t.d_ln_b, dt, M, C, d.eps, stream));
    if (d.inp_u8) {
        RVT_TRY(rvt_stem_wgrad(inp, dy0, t.d_raw_conv, ws_stem, dt, F, d.Cin, d.cin_pad, d.h_raw, d.w_raw, d.H_in, d.W_in, stream));
    } else {
        RVT_TRY(rvt_conv_wgrad(inp, dy0, t.d_raw_conv, ws_wgrad, dt, F, d.H_in, d.W_in, d.cin_pad, C, d.k, d.stride, d.pad, stream));
    }
    if (d_in != nullptr) {
        if (r.conv_dgrad4) {
            RVT_TRY(rvt_conv_dgrad4(dy0, t.conv_wd4, prev_cot, d_in, dt, F, d.H_in, d.W_in, d.cin_pad, C, stream));
        } else {
            RVT_TRY(rvt_conv_dgrad(dy0, t.conv_wd, prev_cot, d_in, dt, F, d.H_in, d.W_in, d.cin_pad, C, d.k, d.stride, d.pad, stream));
        }
    }
    return check_launch("stage_seq_bwd");
}

}  // extern "C"
