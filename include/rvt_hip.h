/* C ABI of librvt_hip.so — the MI355X (gfx950) kernels behind the RVT recurrent backbone.
 *
 * The reference (uzh-rpg/RVT) is pure PyTorch and has no FFI of its own; these entry points are the
 * operator boundary a maintainer would bind.  Each one replaces the ATen op sequence of the
 * cited reference lines.  This header is the ONLY statement of the boundary: the prototypes, the host-side records and
 * the rows of every device table (RvtPackDesc, RvtLayerScaleDesc, RvtOptimChunk, RvtOptimGroup, RvtEventStream) with the
 * enumerators a host needs to fill them are declared here, and so are the records the DEVICE writes and a host only reads back
 * (RvtGradStat, RvtGradStatHead: typedef'd WITHOUT a struct tag, which is how the reader tells the two directions apart);
 * rvt_amd/_header.py derives the ctypes binding and the numpy
 * row layouts from this text, and nothing restates a layout or an argument position elsewhere.  Plain pointers and sizes only:
 *   - every pointer is a DEVICE pointer unless stated otherwise;
 *   - `dtype` selects the storage / MFMA input type of activations and weights:
 *         RVT_F32  (0)  float   — parity mode, exact f32 MFMA
 *         RVT_BF16 (1)  bfloat16 — performance mode
 *     accumulators, LayerNorm/softmax statistics, the LSTM cell state `c`, biases, LayerNorm
 *     affine parameters, LayerScale gammas and ALL gradient outputs of parameters are float32;
 *   - activations are channels-last, token-major: X[frame][y][x][c] with frame = t*B + b;
 *   - `stream` is a hipStream_t; calls are asynchronous, allocate nothing and are graph-capturable;
 *   - return value 0 = ok, non-zero = error (message via rvt_last_error(), thread-local).
 * Channel counts must be multiples of 8; dim_head a multiple of 8 and <= 32; partition size <= 96.
 *
 * TWO TIERS (the operator granularity grew with the tuning history).
 *   Integration surface — what a reference-side maintainer or a non-Python host binds:
 *       rvt_last_error, rvt_tuning_defaults / rvt_get_tuning / rvt_set_tuning          one record of launch geometry + routing
 *       rvt_stage_seq_fwd (+ _ws_bytes)                one call per backbone stage and sequence (no-grad forward)
 *       rvt_stacked_histogram                          event stream -> input tensor (row f4)
 *       rvt_event_sequence (+ _ws_bytes)               B raw event streams -> a whole (T, B, 2*bins, H', W') window sequence, slicing + half-scale
 *       rvt_event_time_repair / rvt_event_decode_dat (+ rvt_event_prep_ws_bytes)   timestamp repair in place; packed Prophesee records -> stream
 *       rvt_mixed_density_stack                        event stream -> the int8 (bins, H, W) mixed-density stack of one window
 *       rvt_event_sequence_mixed (+ _ws_bytes)         B raw event streams -> a whole int8 (T, B, bins, H', W') mixed-density sequence
 *       rvt_yolox_decode / rvt_simota_loss (+ _ws_bytes) / rvt_yolox_decode_bwd        detection tail (row f3)
 *       rvt_yolox_postprocess (+ _ws_bytes)            eval-mode detections -> score filter + batched NMS
 *       rvt_yolox_detect (+ _ws_bytes)                 head maps -> decode + score filter + batched NMS, one launch
 *       rvt_augment_planes / rvt_augment_labels        training-time flip / zoom of event planes and box labels
 *       rvt_frames_pack (+ _ws_bytes) / rvt_frames_unpack   byte planes <-> bitmap + non-zero bytes, unpacked by frame index (the compact store)
 *       rvt_frames_unpack_augment                      packed frames by index -> flipped / zoomed planes, unpack + augmentation in one launch
 *       rvt_frames_gather                              packed frames by address, from device or pinned host stores, into one packed set
 *       rvt_frames_pack2 (+ _ws_bytes) / _unpack2 / _gather2   the same three for format version 2: masks only for non-empty 64-byte groups
 *       rvt_render_preview                             event planes + detection / label boxes -> RGB preview images, one launch
 *       rvt_coco_match / rvt_coco_accumulate (+ _ws_bytes)   detections + labels -> Prophesee / COCO mAP precision table
 *       rvt_coco_recall                                the same records -> true positives below maxDets 1 / 10 / 100, the recall table's numerators
 *       rvt_pack_table                                 all kernel-side weight layouts of a module, one launch per step
 *       rvt_optim_step                                 value clip + AdamW + OneCycle schedule of every parameter, one call per step
 *       rvt_grad_stats (+ _ws_bytes) / rvt_optim_step_guarded   per-tensor gradient statistics + a non-finite verdict into a device ring; the step that obeys it
 *   Operator level — every other entry below: one launch each, what the stage driver sequences and what the Python mirror
 *       (rvt_amd/stage.py, the training backward) calls directly.  Stable and tested one by one (tests/test_kernels.py), but a host
 *       that only runs the model needs none of them; the `*_supported` / `*_ws_*` queries say which fused forms exist for a shape.
 */
#ifndef RVT_HIP_H
#define RVT_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { RVT_F32 = 0, RVT_BF16 = 1 };

const char* rvt_last_error(void);
/* 1 if this library is the CPU SIMT emulator build used by the unit tests, 0 for the gfx950 build */
int rvt_is_emulator(void);

/* Launch geometry and kernel routing, ONE explicit record instead of environment variables (round 4).  The defaults are
 * the production route: what bench.py times and what a deployment runs; nothing in the library reads the environment.
 * The unit tests install a "test geometry" (tiny persistent grids, every kernel family forced on at test-size problems;
 * rvt_amd/tuning.py: TEST_GEOMETRY) through the same call and say so, and the production-route parity tests run on the
 * defaults.  The record is process-wide (not per stream / per thread): set it between launches, not concurrently with them.
 * 0 in a geometry field means "sized by the library" (occupancy query x 256 CUs). */
typedef struct RvtTuning {
    int struct_bytes;         /* sizeof(RvtTuning) of the caller; set / get reject a mismatch */
    /* ---- launch geometry ---- */
    int gemm_resident;        /* persistent workgroups of the 128-row GEMM engine, fused MLP (mlp.hpp) and ConvLSTM scan kernels */
    int wgrad_slice_tokens;   /* minimum tokens per K slice (8192; >= 64) */
    int ppgemm;               /* 1: bf16 products whose shape fits take the 256x256 LDS-DMA kernels (ppgemm.hpp, ppgemm_tn.hpp) */
    int ppgemm_min_m;         /* ... from this many token rows (4096) */
    int ppgemm_all;           /* 1: every epilogue flavour takes ppgemm whatever the contraction length (production: GELU-dual from K >= 512) */
    int ppgemm_grid;          /* workgroups of a ppgemm launch (0 = one per CU, sized by the fullest XCD) */
    int ppgemm_tn_items;      /* token slices per output tile of ppgemm_tn (0 = fill the chip) */
    int one_per_cu_grid;      /* grid cap of the one-workgroup-per-CU kernels: stem forward / weight gradient, chain-MLP weight gradient (0 = 256) */
    int stem;                 /* 1: uint8 planes take the stem kernels (stem.hpp) */
    int mlp_chain;            /* 1: C = 64 MLP halves take the register-chained kernels (mlp_chain.hpp) */
    int mlp_chain_wgrad;      /* 1: ... including the weight-gradient half */
    int chain_resident;       /* persistent workgroups of the chain-MLP / dgrad_ln kernels */
    int dgrad_ln;             /* 1: rvt_linear_dgrad_ln_supported may say yes */
    /* ---- routes taken by the host-side stage driver (rvt_amd/stage.py reads them back through rvt_get_tuning) ---- */
    int route_fused_mlp;      /* -1: by measurement (C = 64 all halves, C = 128 forward); 0: op-by-op; 1: every supported half */
    int route_mlp_bwd_fused;  /* 1: MLP backward recomputed on chip from (dxout, xmid) where built */
    int route_attn_block;     /* 1: fused attention half where built (C = 64) */
    int route_lstm_scan;      /* -1: time loop in the kernel where the weights stay on chip; 0: one launch per step; 1: every built width */
    int route_lstm_scan_wgrad;/* 1: ConvLSTM weight gradients inside the reverse scan where built */
    int route_conv_dgrad4;    /* 1: 3x3 / stride-2 conv input gradient as one gather GEMM */
    int route_stage_driver;   /* 1: the no-grad forward of rvt_amd takes rvt_stage_seq_fwd (one call per stage); 0: the Python host loop */
    int route_mlp_store_pre;  /* 1: the LDS-staged fused MLP forward (C = 128) saves the pre-activation h only, not GELU(h) and GELU'(h); default 0: measured slower (GELU on load costs more than the bytes it saves, profiles/r4/microbench_mlp128.txt) */
    int route_mlp_bwd_both;   /* 1: stage-1 MLP backward = ONE launch (rvt_mlp_bwd_recompute_both) instead of dgrad + wgrad */
    int mlp_stream;           /* 1 (round 5): C = 128 MLP halves take the streamed-weight chain kernels (mlp_stream.hpp): nothing-saved forward,
                                 recompute backward (input-gradient + weight-gradient launch); 0: LDS-staged forward that saves GELU / GELU' + op-by-op backward */
    int ln_linear;            /* 1 (round 5): LayerNorm + qkv projection of a C = 128 block in one launch where rvt_ln_linear_supported, and fc1 + GELU at K = 256, N = 1024 on the weight-stationary kernel (both ln_linear.hpp) */
    int conv_wgrad_tn;        /* 1 (round 5): conv weight gradients with Cout % 256 == 0, Cin % 64 == 0 and k*k*Cin >= 256 take ppgemm_tn.hpp (im2col gather by LDS-DMA; the last 256-wide k tile may lie partly beyond K) */
    int attn_staged;          /* 1 (round 5): the partition-attention core of stages 2-4 stages its rows through LDS (whole-line requests) where built */
    int lstm_scan3;           /* round 6: ConvLSTM (bf16, dws_conv False) with the time loop in the kernel, weights streamed from L2 in operand order, gates saved for the reverse scan (lstm_scan3.hpp): bit 0 = at C 256, bit 1 = at C 128 (instead of lstm_scan.hpp's register-resident weights) */
    int lstm_scan3_rb256;     /* 32-token blocks per workgroup tile of that forward at C = 256: 2 forces 64-token tiles, 1 leaves a stage's choice to rvt_stage_routes (by tokens per step) */
    int lstm_scan3_rb128;     /* ... at C = 128 */
    int route_stage_driver_train; /* 1 (round 6): the training forward / backward of a stage take rvt_stage_seq_train_fwd / rvt_stage_seq_bwd (one call per stage and direction) where covered; 0: the Python host loop */
    int route_attn_preln;     /* 1 (round 6): the backward of a stage's first block also carries the gradient through the down-sampling LayerNorm where no token mask sits between them: rvt_attn_block_bwd_preln on the fused attention half, rvt_linear_dgrad_preln on the op-by-op route (C <= 128); 0: separate rvt_layernorm_bwd */
    int conv_fwd_pp;          /* 1 (round 6): 3 x 3 / stride 2 / pad 1 convs with Cin % 64 == 0 and Cout % 256 == 0 take the 256-wide kernel with the im2col gather in its load stream (ppgemm.hpp GATHER = 2); 0: the 128-row engine */
} RvtTuning;
#define RVT_TUNING_DEFAULTS {(int)sizeof(RvtTuning), 0, 8192, 1, 4096, 0, 0, 0, 0, 1, 1, 1, 0, 1, -1, 1, 1, -1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 3, 1, 1, 1, 1, 1}
void rvt_tuning_defaults(RvtTuning* t);        /* fills *t with the production defaults */
int rvt_get_tuning(RvtTuning* t);              /* t->struct_bytes must be set by the caller */
int rvt_set_tuning(const RvtTuning* t);

/* Measurement aid for bench.py (no reference counterpart): launches `workgroups` x 256 threads that issue nothing but
 * independent v_mfma_f32_32x32x16_bf16 (`iters` x 4 per wave) and returns the FLOPs the launch executes; timed with HIP
 * events it gives the bf16 MFMA rate this part SUSTAINS at its clock under load (the 2.5 PFLOP/s peak assumes 2.4 GHz).
 * scratch: >= workgroups * 256 floats (never written). */
double rvt_probe_mfma(float* scratch, int iters, int workgroups, void* stream);

/* Weight-gradient GEMMs (rvt_*_wgrad) cut the token contraction into K slices.  `ws` is their scratch for the
 * two-stage reduction: rvt_wgrad_workspace_floats(dtype, out_rows, out_cols, tokens, want_colsum) float32 elements
 * (out = dw's [rows][cols]; conv: [Cout][k*k*Cin]; lstm: [4C][2C]).  ws == NULL selects direct float atomics, which
 * are correct but slow on MI355X (device-scope atomics execute memory-side). */
size_t rvt_wgrad_workspace_floats(int dtype, int out_rows, int out_cols, int tokens, int want_colsum);

/* Event-tensor cast + zero pad (modules/detection.py:133-134, utils/padding.py:29-44) fused with the
 * NCHW -> channels-last repack: src [F][Cin][h][w] (src_kind 0: float32, 1: uint8, 2: int8, the planes of the mixed-density
 * stack, which the loader otherwise widens to float32 first: data/genx_utils/sequence_base.py:97-98) ->
 * dst [F][H][W][Cp] (dtype), zero padded to H>=h, W>=w, Cp>=Cin. */
int rvt_prepack_input(const void* src, int src_kind, void* dst, int dtype, int F, int Cin, int h, int w,
                      int H, int W, int Cp, void* stream);

/* Down-sampling conv (maxvit.py:160-168,175; bias-free): in [F][H][W][Cin], w [Cout][k*k*Cin]
 * (tap-major, cin fastest) -> out [F][Ho][Wo][Cout], Ho=(H+2*pad-k)/stride+1.  bf16, k = 3, stride 2, pad 1, even H and W,
 * Cin % 64 == 0, Cout % 256 == 0 (stages 3-4 of RVT-Base): the 256-wide LDS-DMA kernel with the im2col gather in its load
 * stream (tuning.conv_fwd_pp; same products, fp32 summation order of that kernel); everything else: the 128-row engine. */
int rvt_conv_fwd(const void* in, const void* w, void* out, int dtype, int F, int H, int W, int Cin, int Cout,
                 int k, int stride, int pad, void* stream);
/* Input gradient of the 3x3 / stride-2 / pad-1 down-sampling conv of stages 2-4 (reference maxvit.py:160-168, autograd) as ONE
 * product over 2x2 blocks of input pixels (csrc/ppgemm.hpp, GATHER mode).  wd4: [4*Cin][4*Cout] weights in the block-sparse layout
 * of RVT_PACK_CONV_DGRAD4 (below); add (nullable): cotangent already attached to the input, same shape as din.
 * rvt_conv_dgrad4_supported: bf16, k 3, stride 2, pad 1, even H and W, Cin and Cout multiples of 64, enough rows. */
int rvt_conv_dgrad4_supported(int dtype, int H, int W, int Cin, int Cout, int k, int stride, int pad, int F);
int rvt_conv_dgrad4(const void* dy, const void* wd4, const void* add, void* din, int dtype, int F, int H, int W, int Cin, int Cout,
                    void* stream);

/* Input gradient: din[F][H][W][Cin] = conv^T(dy) (+ add).  wd = class-packed transposed weights, see
 * rvt_conv_dgrad_weight_elems / rvt_amd.weights.pack_conv_dgrad: for each parity class (py,px) in
 * row-major order a [Cin][nky*nkx*Cout] matrix.  `add` (nullable) has din's shape. */
int rvt_conv_dgrad(const void* dy, const void* wd, const void* add, void* din, int dtype, int F, int H, int W,
                   int Cin, int Cout, int k, int stride, int pad, void* stream);
/* Weight gradient: dw[Cout][k*k*Cin] (float32) += dy^T im2col(in). */
int rvt_conv_wgrad(const void* in, const void* dy, float* dw, float* ws, int dtype, int F, int H, int W, int Cin,
                   int Cout, int k, int stride, int pad, void* stream);

/* The stem on the loader's uint8 planes (replaces rvt_prepack_input + rvt_conv_fwd + rvt_layernorm_fwd, and
 * rvt_conv_wgrad, for the first stage: maxvit.py:160-177 on the cast + padded input of modules/detection.py:133-134 and
 * utils/padding.py:29-44).  src [F][Cin][h][w] uint8, zero padded to H x W on the fly; w = the packed conv weight of
 * rvt_conv_fwd ([64][7*7*cp], tap-major, cin fastest, cp >= Cin); y0 = conv output, x = LayerNorm(y0), both
 * [F][Ho][Wo][64].  rvt_stem_supported: bf16, uint8 planes, 7x7 / stride 4 / pad 3, Cout = 64, Cin <= 20, w % 4 == 0. */
int rvt_stem_supported(int dtype, int src_u8, int Cin, int Cout, int k, int stride, int pad, int w);
int rvt_stem_fwd(const void* src, const void* w, const float* ln_w, const float* ln_b, void* y0, void* x, int dtype, int F,
                 int Cin, int cp, int h, int wd, int H, int W, float eps, void* stream);
/* dw[64][7*7*cp] (float32, the layout of rvt_conv_wgrad) += dy^T im2col(src); ws: rvt_stem_wgrad_ws_floats floats. */
size_t rvt_stem_wgrad_ws_floats(int Cin, int F, int H, int W);
int rvt_stem_wgrad(const void* src, const void* dy, float* dw, float* ws, int dtype, int F, int Cin, int cp, int h, int wd,
                   int H, int W, void* stream);

/* LayerNorm over channels (maxvit.py:172,177,229,241). */
int rvt_layernorm_fwd(const void* x, const float* w, const float* b, void* y, int dtype, int rows, int C,
                      float eps, void* stream);
/* dx = LN'(dy) (+ dres, nullable);  dw[C] += ..., db[C] += ... */
int rvt_layernorm_bwd(const void* x, const float* w, const void* dy, const void* dres, void* dx, float* dw,
                      float* db, int dtype, int rows, int C, float eps, void* stream);

/* y[M][N] = f(x)[M][K] W[N][K]^T + bias (nullable);  f = exact GELU if gelu_in else identity
 * (maxvit.py:347,353 and the MLP 100-118). */
int rvt_linear_fwd(const void* x, const void* w, const float* bias, void* y, int dtype, int M, int N, int K,
                   int gelu_in, void* stream);
/* MLP fc1 with its activation (maxvit.py:100-112): g = GELU(x W^T + bias) and, if gp != NULL, gp = GELU'(x W^T + bias)
 * (saved for backward so that no kernel re-evaluates erf).  Route note: bf16 at K = 256, N = 1024 (any M) takes the
 * weight-stationary kernel of ln_linear.hpp, whose GELU / GELU' come from the nearest-entry pair table of gelu_lut.hpp
 * (tests/test_kernels.py::test_linear_gelu_weight_stationary); every other shape evaluates erf. */
int rvt_linear_gelu_fwd(const void* x, const void* w, const float* bias, void* g, void* gp, int dtype, int M, int N, int K,
                        void* stream);
/* y = res + gamma * (f(x) W^T + bias)   — LayerScale + residual (maxvit.py:51-53,268-269). */
int rvt_linear_scale_res_fwd(const void* x, const void* w, const float* bias, const float* gamma, const void* res,
                             void* y, int dtype, int M, int N, int K, int gelu_in, void* stream);
/* dx[M][K] = dy[M][N] Wt[K][N]^T, then at most one of:  * gelu'(gelu_pre[M][K]),  + add[M][K],  * mul[M][K]
 * (all nullable). */
int rvt_linear_dgrad(const void* dy, const void* wt, const void* gelu_pre, const void* add, const void* mul, void* dx,
                     int dtype, int M, int N, int K, void* stream);
/* Input gradient of a linear layer whose input is a LayerNorm output, with the LayerNorm backward (+ residual cotangent) in
 * the epilogue (reference maxvit.py:229,347 norm1 -> qkv and :241,100-118 norm2 -> fc1, autograd; csrc/dgrad_ln.hpp):
 *   dx[M][C] = add + LN'(dy[M][K] w[K][C]; x[M][C]),  dln_w[C] += sum_tok (dy w) * xhat,  dln_b[C] += sum_tok (dy w).
 * w = the forward weight in its natural [K][C] layout (compute dtype), add nullable.
 * rvt_linear_dgrad_ln_supported: bf16, C in {64, 128}, K = 3C or 4C. */
int rvt_linear_dgrad_ln_supported(int dtype, int C, int K);
int rvt_linear_dgrad_ln(const void* dy, const void* w, const void* x, const void* add, void* dx, const float* ln_w,
                        float* dln_w, float* dln_b, int dtype, int M, int C, int K, float eps, void* stream);
/* The same launch for a stage's FIRST block (no norm1, maxvit_rnn.py:153), carried through the down-sampling norm in front of it
 * (maxvit.py:177): dy0 = LN'(dy w + add ; y0) - the added cotangent (the block's residual path) enters the norm.  Replaces
 * rvt_linear_dgrad(.., add) + rvt_layernorm_bwd(y0, ..).  Shapes as rvt_linear_dgrad_ln_supported; add is required. */
int rvt_linear_dgrad_preln(const void* dy, const void* w, const void* y0, const void* add, void* dy0, const float* ln_w,
                           float* dln_w, float* dln_b, int dtype, int M, int C, int K, float eps, void* stream);

/* u = LN(x; ln_w, ln_b), y = u W^T + bias in one launch (csrc/ln_linear.hpp; replaces rvt_layernorm_fwd + rvt_linear_fwd for
 * `self.qkv(self.norm1(x))`, reference maxvit.py:268 -> :347).  W [N][C] row-major, bias may be NULL, u may be NULL (no-grad
 * forward: the normalised rows are not kept); ln_w = ln_b = NULL: no LayerNorm (the first block behind a down-sampling conv,
 * maxvit.py:229-236), u is not written.  rvt_ln_linear_supported: bf16, C = 128, N = 384 (tuning.ln_linear = 0: no). */
int rvt_ln_linear_supported(int dtype, int C, int N);
int rvt_ln_linear_fwd(const void* x, const float* ln_w, const float* ln_b, const void* w, const float* bias, void* u, void* y,
                      int dtype, int M, int C, int N, float eps, void* stream);

/* dw[N][K] (float32) += dy[M][N]^T f(x)[M][K];  if dy_colsum != NULL also dy_colsum[N] += column sums of dy
 * (the bias gradient), computed from the tiles the kernel streams anyway. */
int rvt_linear_wgrad(const void* dy, const void* x, float* dw, float* dy_colsum, float* ws, int dtype, int M, int N,
                     int K, int gelu_in, void* stream);

/* Fused MLP half of a block (maxvit.py:269 + :100-118), built for the HBM-bound stages:
 * rvt_mlp_fused_supported(dtype, C) != 0  (bf16: C in {64,128}; f32: C == 64).
 *   rvt_mlp_fwd:  xout = xmid + gamma * (GELU(LN(xmid) W1^T + b1) W2^T + b2) in one pass; if g_out/gp_out are non-NULL
 *                 also g = GELU(h), gp = GELU'(h) [M][4C] for backward; g_out alone (gp_out NULL) receives the PRE-ACTIVATION
 *                 h = LN(xmid) W1^T + b1 instead (half the bytes; the backward applies GELU / GELU' on load through
 *                 rvt_linear_wgrad(gelu_in) and rvt_linear_dgrad(gelu_pre)); and if v2_out is non-NULL the LayerNorm output
 *                 LN(xmid) [M][C] (B operand of the fc1 weight gradient); nothing else of the chain reaches HBM.
 *   rvt_mlp_bwd_dgrad: dh = (dxout (W2*gamma)) * gp;  dxmid = dxout + LN'(dh W1; xmid);  dln_w/dln_b += LayerNorm
 *                 parameter gradients.  w2g_t = (W2*gamma[:,None])^T stored [4C][C]; w1_t = W1^T stored [C][4C].
 * w1 [4C][C], w2 [C][4C] (dtype); ln/bias/gamma and dln_* float32. */
int rvt_mlp_fused_supported(int dtype, int C);
int rvt_mlp_fwd(const void* xmid, void* xout, void* g_out, void* gp_out, void* v2_out, const float* ln_w, const float* ln_b,
                const void* w1, const float* b1, const void* w2, const float* b2, const float* gamma, int dtype, int M,
                int C, float eps, void* stream);
int rvt_mlp_bwd_dgrad(const void* dxout, const void* gp, const void* xmid, void* dh, void* dxmid, const float* ln_w,
                      const void* w2g_t, const void* w1_t, float* dln_w, float* dln_b, int dtype, int M, int C, float eps,
                      void* stream);

/* Backward of the MLP half with NOTHING but the block input saved (rvt_mlp_bwd_fused_supported: C == 64): LN2, fc1, GELU
 * and GELU' are recomputed on chip, and besides dxmid = dxout + LN2'(...) the kernel accumulates the weight gradients in
 * registers across its persistent tile walk:  dw1[4C][C] += dh^T LN2(xmid),  db1[4C] += colsum(dh),
 * s2[C][4C] += dxout^T GELU(h),  cs2[C] += colsum(dxout)  (s2 / cs2 are the RAW fc2 products: LayerScale is folded in by
 * rvt_layerscale_grad_table),  dln_w / dln_b += LayerNorm parameter gradients.  w1 [4C][C]; w2g_t = (W2*gamma[:,None])^T
 * [4C][C]; w1_t = W1^T [C][4C].  ws: rvt_mlp_bwd_fused_ws_floats(dtype, C, M) floats (per-workgroup partials). */
int rvt_mlp_bwd_fused_supported(int dtype, int C);
size_t rvt_mlp_bwd_fused_ws_floats(int dtype, int C, int M);
/* The same kernel cut in two along the critical path of backward (both recompute LN2 / fc1 / GELU from xmid):
 *   rvt_mlp_bwd_recompute_dgrad: dxmid and dln_w / dln_b only — no weight-gradient accumulators, several workgroups per CU;
 *   rvt_mlp_bwd_recompute_wgrad: dw1, db1, s2, cs2 only (two groups of hidden chunks per tile column, 64 accumulator
 *     registers each) — for the weight-gradient stream; reads (dxout, xmid) once per group instead of the 10 rows of C
 *     per token the two weight-gradient GEMMs re-read. */
int rvt_mlp_bwd_recompute_dgrad(const void* dxout, const void* xmid, void* dxmid, const float* ln_w, const float* ln_b,
                                const void* w1, const float* b1, const void* w2g_t, const void* w1_t, float* dln_w,
                                float* dln_b, int dtype, int M, int C, float eps, void* stream);
int rvt_mlp_bwd_recompute_wgrad(const void* dxout, const void* xmid, const float* ln_w, const float* ln_b, const void* w1,
                                const float* b1, const void* w2g_t, float* dw1, float* db1, float* s2, float* cs2, float* ws,
                                int dtype, int M, int C, float eps, void* stream);
/* Round 4: both of the above in ONE launch where rvt_mlp_bwd_both_supported (bf16, C = 64, RvtTuning.route_mlp_bwd_both): the
 * weight-gradient kernel's dh tile goes through LDS to two rotating waves that form dh W1, and the LayerNorm backward + residual
 * runs in the staging role of all threads — one recompute of fc1 / GELU / GELU' and one read of xmid / dxout instead of two. */
int rvt_mlp_bwd_both_supported(int dtype, int C);
int rvt_mlp_bwd_recompute_both(const void* dxout, const void* xmid, void* dxmid, const float* ln_w, const float* ln_b, const void* w1,
                               const float* b1, const void* w2g_t, const void* w1_t, float* dln_w, float* dln_b, float* dw1, float* db1,
                               float* s2, float* cs2, float* ws, int dtype, int M, int C, float eps, void* stream);

/* Partitioned multi-head attention core (maxvit.py:252-265,273-304,343-354 minus the two linears):
 * qkv [F*H*W][3C] in image token order, per-head layout [q|k|v]; out [F*H*W][C].  window=1: ph x pw
 * windows; window=0: dilated grid with grid size (ph,pw). */
int rvt_attn_fwd(const void* qkv, void* out, int dtype, int F, int H, int W, int C, int dim_head, int ph, int pw,
                 int window, void* stream);
int rvt_attn_bwd(const void* qkv, const void* dout, void* dqkv, int dtype, int F, int H, int W, int C, int dim_head,
                 int ph, int pw, int window, void* stream);

/* Fused attention half of a PartitionAttentionCl block (replaces maxvit.py:268 = norm1 :229, SelfAttentionCl :343-354 on
 * the partitions of :273-304, LayerScale :51-53 and the residual): one wave per partition, everything between the x rows
 * and the xmid rows on chip (csrc/attn_block.hpp).  rvt_attn_block_supported: C == 64, dim_head == 32, 32 < ph*pw <= 96.
 *   fwd: xmid = x + gamma * (attention(LN1(x) wqkv^T + bqkv) wp^T + bp); ln_w / ln_b NULL = no norm1 (first window block of a
 *        stage, maxvit_rnn.py:153); a_out (nullable) receives the attention output rows [F*H*W][C] (operand of the proj
 *        weight gradient).  wqkv [3C][C] (rows [head][q|k|v][dh]), wp [C][C].
 *   bwd: dx = dxmid + LN1'(dqkv wqkv), dqkv = attention backward of dxmid (gamma wp) with q / k / v / P recomputed from x;
 *        writes dqkv [F*H*W][3C] and (u_out nullable, LN only) LN1(x) for the qkv weight-gradient GEMM; dln_w / dln_b +=
 *        LayerNorm parameter gradients.  wpg_t = (wp * gamma[:,None])^T [C][C]. */
int rvt_attn_block_supported(int dtype, int C, int dim_head, int L);
int rvt_attn_block_fwd(const void* x, void* xmid, void* a_out, const float* ln_w, const float* ln_b, const void* wqkv,
                       const float* bqkv, const void* wp, const float* bp, const float* gamma, int dtype, int F, int H, int W,
                       int C, int dim_head, int ph, int pw, int window, float eps, void* stream);
int rvt_attn_block_bwd(const void* x, const void* dxmid, void* dx, void* dqkv, void* u_out, const float* ln_w,
                       const float* ln_b, const void* wqkv, const float* bqkv, const void* wpg_t, float* dln_w, float* dln_b,
                       int dtype, int F, int H, int W, int C, int dim_head, int ph, int pw, int window, float eps,
                       void* stream);
/* The backward of a stage's FIRST block (no norm1: its input x = LN_pre(y0) is the output of the down-sampling norm,
 * maxvit.py:177, maxvit_rnn.py:153) carried through that norm in the same launch (round 6): dy0 = LN_pre'(dxmid + dqkv wqkv ; y0)
 * is written instead of dx, ln_w is LN_pre's weight, dln_w / dln_b += its parameter gradients (autograd of maxvit.py:177).
 * Replaces rvt_attn_block_bwd(ln_w = NULL) followed by rvt_layernorm_bwd(y0, ..): same dqkv bits, one row per token less to
 * write and two less to read.  Partitions of at most 64 tokens (two 32-token blocks), like rvt_attn_block_bwd. */
int rvt_attn_block_bwd_preln(const void* x, const void* y0, const void* dxmid, void* dy0, void* dqkv, const float* ln_w,
                             const void* wqkv, const float* bqkv, const void* wpg_t, float* dln_w, float* dln_b, int dtype, int F,
                             int H, int W, int C, int dim_head, int ph, int pw, int window, float eps, void* stream);

/* ConvLSTM cell with 1x1 conv (rnn.py:52-67): mix = [x|h_prev] Wp^T + bp with gate-interleaved rows
 * (row n' = (c/8)*32 + gate*8 + c%8, gates f,i,o,g); writes h_out [M][C], c_out [M][C] (float32) and,
 * if gates != NULL, the activated gates [M][4C] in natural order [f|i|o|g]. */
int rvt_lstm_fwd(const void* x, const void* h_prev, const float* c_prev, const void* w_perm, const float* b_perm,
                 void* h_out, float* c_out, void* gates, int dtype, int M, int C, void* stream);
/* BPTT element-wise part: consumes dh_in (+ dh_rec nullable), updates dc_rec in place, writes dz [M][4C]. */
int rvt_lstm_gates_bwd(const void* dh_in, const void* dh_rec, float* dc_rec, const void* gates, const float* c_new,
                       const float* c_prev, void* dz, int dtype, int M, int C, void* stream);
/* [dx | dh_rec] = dz W : wt = W^T [2C][4C] natural gate order. */
int rvt_lstm_dgrad(const void* dz, const void* wt, void* dx, void* dh_rec, int dtype, int M, int C, void* stream);
/* dw[4C][2C] (float32) += dz^T [x | h_prev];  dz_colsum[4C] += column sums of dz if non-NULL (bias gradient). */
int rvt_lstm_wgrad(const void* dz, const void* x, const void* h_prev, float* dw, float* dz_colsum, float* ws, int dtype,
                   int M, int C, void* stream);

/* The same ConvLSTM cell (rnn.py:43-67) with the TIME LOOP INSIDE the kernel, for the 1x1-conv variant (dws_conv False: the
 * recurrence is independent per pixel): one launch per stage runs all T_steps of modules/detection.py:131-148 for that stage
 * with h / c on chip.  rvt_lstm_scan_supported(dtype, C) != 0 for C in {32, 64, 128}.
 *   fwd: x_all [T][M][C]; Hall [T+1][M][C], slot 0 = incoming h (caller-filled), slots 1..T written; c0 fp32 [M][C] or
 *        NULL (zeros); c_last fp32 [M][C]; Csave [T][M][C] (dtype; slot t = c_t, what BPTT needs) or NULL (inference);
 *        w [4C][2C] in the reference's NATURAL order (rows f,i,o,g; columns [x|h]); bias fp32 [4C].
 *   bwd: reverse scan with the gates recomputed; dH [T][M][C] cotangent of Hall[1..] (NULL = zeros), dc_last fp32 [M][C]
 *        (NULL = zeros); wt = w^T [2C][4C]; writes dx_all [T][M][C], dz_all [T][M][4C] (pre-activation gradients, natural
 *        gate order, operand of rvt_lstm_wgrad), dh0 [M][C], dc0 fp32 [M][C]. */
int rvt_lstm_scan_supported(int dtype, int C);
/*        bf16, C = 128 (rvt_lstm_scan_saves_gates): the weights live in the register file; with gates_out != NULL the forward
 *        also stores the activated gates [T][M][4C] (natural order f,i,o,g), and the backward given `gates` reads them instead
 *        of recomputing (W^T in registers; x_all / Hall unused; dz_all written for rvt_lstm_wgrad). */
int rvt_lstm_scan_saves_gates(int dtype, int C);
int rvt_lstm_scan_fwd(const void* x_all, void* Hall, const float* c0, float* c_last, void* Csave, const void* w,
                      const float* bias, void* gates_out, int dtype, int M, int C, int T_steps, void* stream);
/*        With dw != NULL (rvt_lstm_scan_bwd_ws_floats(dtype, C, M) > 0: bf16, C <= 64) the weight gradients are accumulated
 *        inside the kernel: dw [4C][2C] += dz^T [x | h_prev], db [4C] += colsum(dz) (natural gate order, fp32), through
 *        per-workgroup partial records in ws; dz_all is then neither written nor needed (may be NULL). */
size_t rvt_lstm_scan_bwd_ws_floats(int dtype, int C, int M);
int rvt_lstm_scan_bwd(const void* x_all, const void* Hall, const void* Csave, const float* c0, const void* dH,
                      const float* dc_last, const void* w, const void* wt, const float* bias, void* dx_all, void* dz_all,
                      void* dh0, float* dc0, float* dw, float* db, float* ws, const void* gates, int dtype, int M, int C,
                      int T_steps, void* stream);

/* ---- ConvLSTM of the WIDE stages with the time loop in the kernel (csrc/lstm_scan3.hpp; reference models/layers/rnn.py:43-67 over
 * the loop of modules/detection.py:131-148, and its BPTT).  bf16, dws_conv False, C = 128 / 256 (rvt_lstm_scan3_supported).  The weights do
 * not fit on chip: they are streamed from L2 every step in MFMA-operand order, which rvt_lstm_scan3_pack produces once per
 * optimizer step from the natural [4C][2C] matrix (gate order f,i,o,g, input order [x | h]: rnn.py:52-61):
 *   wp_fwd  [C/32][2C/16][4][64][8]   (wave = 32-channel block, k-step, gate, lane, element)        = 4C * 2C elements
 *   wtp_bwd [C/32][4C/16][2][64][8]   (wave = 32-channel block, k-step, x | h part, lane, element)  = rows of W^T, same size
 * Forward: x_all [T][M][C], Hall [T+1][M][C] (slot 0 = incoming h, filled by the caller; slots 1.. written), c0 fp32 [M][C] or
 * NULL (zeros, rnn.py:43-47), c_last fp32 [M][C].  For BPTT it saves the ACTIVATED gates (gsave) and a bf16 copy of the cell
 * states (Csave) in a private register-dump order; both buffers hold T * rvt_lstm_scan3_rows(C, M) * 4C / * C elements and are
 * NULL together for a no-grad forward.  Backward: reads them back (same M, same rb), dH [T][M][C] = cotangent of Hall[1..]
 * (NULL = zeros), dc_last fp32 [M][C] (NULL = zeros); writes dx_all [T][M][C], dz_all [T][M][4C] (natural gate order: the operand
 * of rvt_lstm_wgrad), dh0 [M][C], dc0 fp32 [M][C]. */
int rvt_lstm_scan3_supported(int dtype, int C);
/* rb in {1, 2}: the forward walks tiles of 32 * rb tokens, and the number of 32-token blocks the dumps hold per step depends on it,
 * so ONE value serves the buffer sizing, the forward and the reverse scan of a step (the reverse scan's own tile is the launcher's
 * choice and independent of it).  rvt_lstm_scan3_rb(C) is the tuned value (RvtTuning.lstm_scan3_rb128 / _rb256); a stage takes rb from
 * its route record (RvtStageRoutes.lstm_scan3_rb: 2 where the tuned value is 2 or the stage has Ms * C >= 2^22 token-channels per
 * step, else 1), never from the tuning record a second time. */
int rvt_lstm_scan3_rb(int C);
int rvt_lstm_scan3_rows(int C, int M, int rb);
int rvt_lstm_scan3_pack(const void* w, void* wp_fwd, void* wtp_bwd, int C, void* stream);
int rvt_lstm_scan3_fwd(const void* x_all, void* Hall, const float* c0, float* c_last, void* Csave, const void* wp, const float* bias,
                       void* gsave, int dtype, int M, int C, int T_steps, int rb, void* stream);
int rvt_lstm_scan3_bwd(const void* gsave, const void* Csave, const float* c0, const void* dH, const float* dc_last, const void* wtp,
                       void* dx_all, void* dz_all, void* dh0, float* dc0, int dtype, int M, int C, int T_steps, int rb, void* stream);

/* ---- stage-major driver (rvt_stage_seq_fwd) -------------------------------------------------------------
 * One backbone stage (reference maxvit_rnn.py:169-182: down-sampling conv + LayerNorm, the window and grid attention blocks,
 * the ConvLSTM) over ALL T time steps of B sequences in ONE call, for the NO-GRAD forward: validation and streaming inference
 * (modules/detection.py:231-255 with T = 1 per call).  The driver asks rvt_stage_routes (below) for the stage's routes and runs the
 * block loop and the ConvLSTM loop that rvt_amd/stage.py's host loop runs in Python; it launches exactly the operators declared in
 * this header, on `stream`.  (The training forward / backward have a driver of their own further down: rvt_stage_seq_train_fwd.)
 * All pointers in the descriptors are DEVICE pointers except `blocks`, a HOST array of 2 * num_blocks records
 * (window block, grid block, window, grid, ...).  Unsupported here (call the operators instead): token masks, DWS-ConvLSTM. */
typedef struct RvtBlockWeights {          /* one PartitionAttentionCl block, maxvit.py:193-270 */
    const float *n1_w, *n1_b;             /* norm1 (NULL, NULL: Identity - the first window block of a stage) */
    const void* qkv_w; const float* qkv_b;      /* [3C][C] (dtype), [3C] */
    const void* proj_w; const float* proj_b;    /* [C][C], [C] */
    const float* g1;                      /* LayerScale 1 [C] */
    const float *n2_w, *n2_b;             /* norm2 */
    const void* fc1_w; const float* fc1_b;      /* [4C][C], [4C] */
    const void* fc2_w; const float* fc2_b;      /* [C][4C], [C] */
    const float* g2;                      /* LayerScale 2 [C] */
} RvtBlockWeights;
typedef struct RvtStageDesc {
    int struct_bytes;                     /* sizeof(RvtStageDesc) */
    int dtype, C, Cin, cin_pad;           /* cin_pad: channel count of the packed conv weight / prepacked input (multiple of 8) */
    int H_in, W_in, k, stride, pad;       /* conv geometry on the (padded) input resolution */
    int ph, pw, dim_head, num_blocks;
    float eps;
    int inp_u8, h_raw, w_raw;             /* stage 1 fed by the loader's uint8 planes [F][Cin][h_raw][w_raw] (cast + zero pad fused in) */
    const void* conv_w;                   /* [C][k*k*cin_pad] tap-major (rvt_conv_fwd layout) */
    const float *ln_w, *ln_b;             /* LayerNorm after the conv */
    const RvtBlockWeights* blocks;        /* HOST array, 2 * num_blocks entries */
    const void* lstm_w; const float* lstm_b;      /* gate-interleaved rows (rvt_lstm_fwd) */
    const void* lstm_wn; const float* lstm_bn;    /* natural row order (rvt_lstm_scan_fwd) */
} RvtStageDesc;
/* inp: [T*B][H_in][W_in][cin_pad] channels-last (dtype), or the uint8 planes when inp_u8;  h0 [B][H][W][C] (dtype) / c0 fp32,
 * both NULL = zero state;  Hall [T+1][B][H][W][C]: slot 0 is scratch for the incoming h, slots 1..T receive h_t (the stage's
 * output features = the next stage's input);  c_last fp32 [B][H][W][C];  ws: rvt_stage_seq_fwd_ws_bytes(desc, T, B) bytes.
 * The size is the driver's own carve run without a base pointer (256-byte pieces, only those the routes use, plus 256 bytes for a base
 * of any alignment): it depends on the tuning record through the routes, so ask again after rvt_set_tuning.  A smaller ws is refused
 * before anything is launched. */
size_t rvt_stage_seq_fwd_ws_bytes(const RvtStageDesc* desc, int T, int B);
int rvt_stage_seq_fwd(const RvtStageDesc* desc, const void* inp, const void* h0, const float* c0, void* Hall, float* c_last,
                      void* ws, size_t ws_bytes, int T, int B, void* stream);

/* ---- the routes of one stage ---------------------------------------------------------------------------------------------------
 * Which kernels a stage runs, decided ONCE per forward by rvt_stage_routes from (tuning record, rvt_*_supported answers, shape) and
 * carried with the saved activations: the backward of a training step reads the record its forward was planned with, never the
 * tuning record again.  Consumers: rvt_stage_seq_fwd (plans internally), RvtStageTrain below, the host loop of rvt_amd/stage.py. */
typedef struct RvtStageRoutes {
    int attn_block;                       /* 1: fused attention half (rvt_attn_block_fwd / _bwd) */
    int ln_linear;                        /* 1: norm1 + qkv in one launch (rvt_ln_linear_fwd); implies attn_block = 0 */
    int mlp_route;                        /* 0: LayerNorm, fc1 + GELU / GELU', fc2 as separate launches; 1: recompute route (rvt_mlp_fwd keeps nothing);
                                             2: rvt_mlp_fwd saving what an op-by-op style backward reads (host loop only; save = 1 only) */
    int mlp_bwd_both;                     /* route 1: rvt_mlp_bwd_recompute_both instead of _dgrad + _wgrad */
    int dgrad_ln_qkv, dgrad_ln_fc1;       /* 1: that input gradient + the LayerNorm backward behind it in one launch (rvt_linear_dgrad_ln) */
    int lstm_route;                       /* 0: one launch per step; 1: the rvt_lstm_scan_ kernels, gates recomputed; 2: the same with saved gates; 3: the rvt_lstm_scan3_ kernels */
    int lstm_scan_wgrad;                  /* route 1: ConvLSTM weight gradients inside the reverse scan */
    int conv_dgrad4;                      /* 1: rvt_conv_dgrad4 for the input gradient of the down-sampling conv (where the host built its weight copy) */
    int attn_preln;                       /* the first block's backward also carries the gradient through the down-sampling norm: rvt_attn_block_bwd_preln (attn_block = 1) or rvt_linear_dgrad_preln (dgrad_ln_qkv = 1) */
    int mlp_store_pre;                    /* route 2: keep the pre-activation h alone; GELU / GELU' are applied on load by the backward */
    int mlp_bwd_dgrad;                    /* route 2: both MLP input gradients + the norm2 backward in one launch (rvt_mlp_bwd_dgrad) */
    int lstm_scan3_rb;                    /* route 3: the tile factor of forward, dump buffers and reverse scan (1 or 2); 0 otherwise */
    int driver_covers;                    /* 1: the C-side driver of this direction runs these routes (no token mask, no DWS-ConvLSTM; training:
                                             also mlp_route != 2); 0: the host loop does */
} RvtStageRoutes;
/* save: the forward keeps activations for a backward.  has_dws / has_token_mask: the stage has a DWS-ConvLSTM / a token mask is applied. */
int rvt_stage_routes(const RvtStageDesc* desc, int T, int B, int save, int has_dws, int has_token_mask, RvtStageRoutes* out);

/* ---- training-side stage driver (rvt_stage_seq_bwd; round 6) ----------------------------------------------
 * The TRAINING forward and the BPTT backward of one stage (reference maxvit_rnn.py:169-182 under autograd, driven by
 * modules/detection.py:131-148) as ONE library call each: the per-operator launches that rvt_amd/stage.py issued from Python
 * (40 - 150 per stage and direction) are sequenced here.  Division of labour: rvt_stage_routes decides the kernel routes; the HOST
 * copies that record into `routes` and owns every tensor that outlives the call - the activations kept for backward (RvtBlockSaved and
 * the stage-level pointers below) and the gradient buckets; the driver owns the order of launches and the backward's temporaries
 * (carved from `ws`).  Nothing is launched that the operator entry points above do not launch.  Not covered (the host keeps its
 * operator-by-operator loop, rvt_amd/stage.py): whatever routes.driver_covers = 0 stands for. */
typedef struct RvtBlockSaved {            /* activations of one block kept for backward; NULL = not kept on the chosen route */
    const void* xin;                      /* block input [M][C] (= previous block's xout, or the LayerNorm output of the down-sampling) */
    void* u;                              /* norm1(xin) (op-by-op attention with a norm1) */
    void* qkv;                            /* [M][3C] (op-by-op attention) */
    void* a;                              /* attention output rows [M][C] (operand of the proj weight gradient) */
    void* xmid;                           /* [M][C] */
    void* v2;                             /* norm2(xmid) (op-by-op MLP) */
    void* hg; void* hgp;                  /* GELU(h), GELU'(h) [M][4C] (op-by-op MLP) */
    void* xout;                           /* [M][C] */
} RvtBlockSaved;
typedef struct RvtBlockTrain {            /* backward-side operands and fp32 gradient accumulators (+=) of one block */
    const void *qkv_wt, *proj_wt, *fc1_wt, *fc2_wt;      /* W^T copies; proj / fc2 with LayerScale folded in (rvt_amd/weights.py) */
    float *d_n1_w, *d_n1_b;               /* NULL without norm1 */
    float *d_qkv_w, *d_qkv_b, *d_S1, *d_cs1;             /* S1 = dxmid^T a, cs1 = colsum(dxmid): raw proj products (LayerScale fold later) */
    float *d_n2_w, *d_n2_b, *d_fc1_w, *d_fc1_b, *d_S2, *d_cs2;
} RvtBlockTrain;
typedef struct RvtStageTrain {
    int struct_bytes;                     /* sizeof(RvtStageTrain) */
    RvtStageRoutes routes;                /* as rvt_stage_routes(.., save = 1, ..) filled it for the forward; the backward reads the same record */
    const RvtBlockSaved* saved;           /* HOST arrays, 2 * num_blocks entries each */
    const RvtBlockTrain* tb;
    void *y0, *x0;                        /* conv output, LayerNorm output (= saved[0].xin) */
    void* Hall;                           /* [T+1][B][H][W][C]; slot 0 = incoming h, filled by the host */
    float* c_last;                        /* [B][H][W][C] */
    void* Csave;                          /* scan routes: cell-state copies (layout of the scan kernel in use) */
    void* gates;                          /* routes 0, 2, 3: activated gates */
    float* Call;                          /* route 0: [T+1][B][H][W][C] fp32; slot 0 = incoming c, filled by the host */
    const float* c0_saved;                /* scan routes, backward: the incoming cell state as the forward saw it (NULL = zeros) */
    const void *lstm_wp3, *lstm_wtp3;     /* route 3: rvt_lstm_scan3_pack outputs */
    const void *lstm_wt, *conv_wd4, *conv_wd;
    float *d_lstm_w, *d_lstm_b, *d_ln_w, *d_ln_b, *d_raw_conv;
} RvtStageTrain;
/* inp / h0 / c0 as rvt_stage_seq_fwd.  No workspace: every buffer the forward writes is named in `tr`. */
int rvt_stage_seq_train_fwd(const RvtStageDesc* desc, const RvtStageTrain* tr, const void* inp, const float* c0, int T, int B,
                            void* stream);
/* dH [T][B][H][W][C] cotangent of Hall[1..] (route 0: must not be NULL), dc_last fp32 (NULL = zeros), prev_cot: cotangent already
 * attached to the stage's input frames (added to the conv input gradient; NULL = none), d_in [T*B][H_in][W_in][Cin] (NULL: no
 * input gradient), dh0 [B][H][W][C], dc0 fp32.  `inp` = the tensor the forward read (planes or channels-last frames).
 * ws: rvt_stage_seq_bwd_ws_bytes bytes - the backward's own carve run without a base pointer (2-MiB pieces plus 2 MiB for a base of
 * any alignment; it reads tr->routes, not the tuning record); a smaller ws is refused before anything is launched.
 * Parameter gradients are ACCUMULATED (+=) into the pointers of `tr`. */
size_t rvt_stage_seq_bwd_ws_bytes(const RvtStageDesc* desc, const RvtStageTrain* tr, int T, int B);
int rvt_stage_seq_bwd(const RvtStageDesc* desc, const RvtStageTrain* tr, const void* inp, const void* dH, const float* dc_last,
                      const void* prev_cot, void* d_in, void* dh0, float* dc0, void* ws, size_t ws_bytes, int T, int B, void* stream);

/* Depth-wise k x k conv (k = 3; groups = channels, padding k/2, stride 1) of the DWS-ConvLSTM (rnn.py:25-29,50-54)
 * on channels-last maps: y[n][y][x][c] = b[c] + sum_taps w[c][ky][kx] x[...][c].  x / y rows have pitch ldx / ldy
 * elements (so a C-wide slice of a 2C-wide buffer can be addressed).  transpose=1 computes the input gradient
 * (mirrored taps, bias ignored).  w: float32 [C][k*k], b: float32 [C]. */
int rvt_dwconv_fwd(const void* x, int ldx, const float* w, const float* b, void* y, int ldy, int dtype, int N, int H,
                   int W, int C, int k, int transpose, void* stream);
/* dw[C][k*k] += correlate(x, dy), db[C] += sum dy  (float32). */
int rvt_dwconv_wgrad(const void* x, int ldx, const void* dy, int ldy, float* dw, float* db, int dtype, int N, int H,
                     int W, int C, int k, void* stream);

/* Token masking of stage 1 (maxvit_rnn.py:174-176): rows of x[M][C] with mask[m] != 0 are overwritten by the float32
 * mask token;  backward: dtoken[C] += sum of dx over masked rows, and those rows of dx are zeroed in place. */
int rvt_token_mask_fwd(void* x, const unsigned char* mask, const float* token, int dtype, int M, int C, void* stream);
int rvt_token_mask_bwd(void* dx, const unsigned char* mask, float* dtoken, int dtype, int M, int C, void* stream);

/* Labelled-frame gather of the training step (modules/utils/detection.py:32-46, BackboneFeatureSelector): dst[n] = src[idx[n]]
 * over whole frames of frame_bytes (a multiple of 16) for n < n_sel; idx: int32 frame indices (t*B + b), on the device.
 * scatter = 1 is the backward: dst[idx[n]] = src[n] (dst zero-filled by the caller; indices distinct). */
int rvt_gather_frames(const void* src, const int* idx, void* dst, int n_sel, size_t frame_bytes, int scatter, void* stream);

/* ---- YOLOX PAFPN building block (reference models/detection/yolox/models/network_blocks.py:29-53) ----
 * BaseConv = Conv2d(bias=False) -> BatchNorm2d(eps 1e-5, momentum 0.1) -> SiLU on channels-last maps x[rows = N*H*W][C].  The conv
 * is rvt_conv_fwd / rvt_conv_dgrad / rvt_conv_wgrad; these are the row-wise kernels around it (csrc/bnact.hpp).  act: 0 none, 1 SiLU.
 *   rvt_bn_stats:          stats[2][C] in fp64 (zero it first): stats[0] += column sums of x, stats[1] += column sums of x^2.  fp64 because
 *                          var = E[x^2] - mean^2 taken in fp32 cancels when |mean| >> std; under data parallelism these two vectors
 *                          are what SyncBatchNorm all-reduces, train.py:133
 *   rvt_bn_finalize:       training: mean = stats[0] / rows, var = stats[1] / rows - mean^2 (biased, in fp64), running statistics
 *                          updated in place with `momentum` (unbiased variance) when non-NULL; eval (stats may be NULL): mean / var =
 *                          the running statistics.  Writes
 *                          scale = gamma * rstd, shift = beta - mean * scale and (nullable) mean_out / rstd_out for the backward.
 *   rvt_bn_act_fwd:        y = act(x * scale + shift)            (y may alias x)
 *   rvt_bn_act_bwd_stats:  dz = dy * act'(x * scale + shift);  dsum[C] += sum dz (= dbeta), dxsum[C] += sum dz * xhat (= dgamma), fp64 like
 *                          every column sum here (thousands of workgroups' partial sums meet in one word per channel)
 *   rvt_bn_act_bwd_apply:  dx = scale * (dz - dsum / rows - xhat * dxsum / rows)      (training-mode BatchNorm backward) */
/* Inference: Conv2d(bias=False) + BatchNorm2d (running statistics) + activation in ONE launch — scale / shift from rvt_bn_finalize
 * (training = 0) applied to the fp32 accumulator in the GEMM epilogue; act 0 = none, 1 = SiLU.  in / w / out as rvt_conv_fwd. */
int rvt_conv_bn_act_fwd(const void* in, const void* w, const float* scale, const float* shift, void* out, int dtype, int F, int H, int W,
                        int Cin, int Cout, int k, int stride, int pad, int act, void* stream);
int rvt_bn_stats(const void* x, double* stats, int dtype, int rows, int C, void* stream);
int rvt_bn_finalize(const double* stats, int rows, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                    float* running_var, float* mean_out, float* rstd_out, float* scale, float* shift, int C, int training, void* stream);
int rvt_bn_act_fwd(const void* x, const float* scale, const float* shift, void* y, int dtype, int rows, int C, int act, void* stream);
/* rvt_bn_finalize (training) + rvt_bn_act_fwd in ONE launch: count = rows the sums cover (the global count under synchronised BatchNorm) */
int rvt_bn_train_act_fwd(const void* x, const double* stats, int count, const float* gamma, const float* beta, float eps, float momentum,
                         float* running_mean, float* running_var, float* mean_out, float* rstd_out, float* scale_out, float* shift_out,
                         void* y, int dtype, int rows, int C, int act, void* stream);
int rvt_bn_act_bwd_stats(const void* dy, const void* x, const float* scale, const float* shift, const float* mean, const float* rstd,
                         double* dsum, double* dxsum, int dtype, int rows, int C, int act, void* stream);
int rvt_bn_act_bwd_apply(const void* dy, const void* x, const float* scale, const float* shift, const float* mean, const float* rstd,
                         const double* dsum, const double* dxsum, void* dx, int dtype, int rows, int C, int act, void* stream);

/* YOLOX head tail on [B][A][5 + num_classes] fp32 prediction tensors (rvt_amd/csrc/simota.hpp; host mirror rvt_amd/head.py).
 * Replaces models/detection/yolox/models/yolo_head.py:236-290 (decode) and :291-606 (get_losses / get_assignments /
 * simota_matching: the per-image Python loop with its int(nlabel[b]) / .item() host syncs and per-ground-truth topk) by a fixed
 * sequence of launches with no host synchronisation.  Anchors are ordered level by level, row-major inside a level.
 *   rvt_yolox_decode:     one FPN level.  reg_obj [B*H*W][ld_ro] (columns 0-3 box regression, 4 objectness logit) and
 *                         cls [B*H*W][ld_cls] (class logits) of `dtype` -> rows anchor_offset.. of pred_train (decoded cx cy w h,
 *                         raw logits; NULL = skip) and pred_infer (decoded box, sigmoid scores; NULL = skip), both [B][A][5+nc].
 *   rvt_yolox_decode_bwd: d_reg_obj / d_cls = gradient of pred_train's rows of this level, columns scaled by
 *                         col_scale[0] (box) / [1] (objectness) / [2] (class) read from DEVICE memory; padding columns zeroed.
 *   rvt_simota_loss:      labels [B][G][5] fp32 rows (class, cx, cy, w, h), zero rows = padding AFTER the real ones (:309).
 *                         losses[5] (device) = loss, 5 * iou loss, objectness loss, class loss, num_fg / max(num_gts, 1);
 *                         g_pred (NULL = skip) = d(sum iou) / d box, d(sum obj) / d objectness, d(sum cls) / d class, each divided
 *                         by max(num_fg, 1): the caller scales the three column groups (5 * dloss + d(iou loss) ...);
 *                         match_out [B][A] (NULL = skip) = matched ground-truth row or -1, piou_out [B][A] = IoU with it.
 *                         use_l1 (an option no RVT config turns on) is not implemented. */
int rvt_yolox_decode(const void* reg_obj, const void* cls, int ld_ro, int ld_cls, int dtype, int B, int H, int W, int stride,
                     int num_classes, int anchor_offset, int A, float* pred_train, float* pred_infer, void* stream);
int rvt_yolox_decode_bwd(const float* g_pred, const float* pred_train, const float* col_scale, void* d_reg_obj, void* d_cls, int ld_ro,
                         int ld_cls, int dtype, int B, int H, int W, int stride, int num_classes, int anchor_offset, int A, void* stream);
size_t rvt_simota_ws_bytes(int B, int G, int A);
int rvt_simota_loss(const float* pred_train, const float* labels, const int* level_hw, const int* level_stride, int L, int B, int G, int A,
                    int num_classes, float* losses, float* g_pred, int* match_out, float* piou_out, void* ws, size_t ws_bytes,
                    void* stream);

/* Detection post-processing of the eval-mode detections (rvt_amd/csrc/nms.hpp; host mirror rvt_amd/postprocess.py).  Replaces
 * models/detection/yolox/utils/boxes.py:32-76 (`postprocess`: a Python loop over the images, boolean-mask indexing and
 * torchvision's NMS) by ONE launch for the whole batch with no host synchronisation and no device-to-host copy: capturable.
 *   pred [B][A][5+nc] fp32 rows cx cy w h obj cls... (the pred_infer of rvt_yolox_decode); it is only read.
 *   Per image: class_conf = max over the class columns, class_pred = its index (lowest index on an exact tie);
 *   score = obj * class_conf (one fp32 multiply); candidates are the anchors with score >= conf_thre, ordered by descending
 *   score, the lower anchor first on an exact tie; greedy NMS in that order: a candidate still alive is kept and kills every
 *   later candidate of the same class (of any class if class_agnostic) whose IoU with it is > nms_thre.  Corners are
 *   cx -+ w/2, cy -+ h/2; area = (x2-x1)*(y2-y1); inter = max(0, min(x2)-max(x1)) * max(0, min(y2)-max(y1));
 *   iou = inter / (area_a + area_b - inter) in fp32 in exactly this order (torchvision's CPU kernel, no "+1"); a pair whose
 *   union is not positive never suppresses.  Every keep / kill decision equals the same formula evaluated by torch.
 *   det [B][max_det][7] = x1 y1 x2 y2 obj class_conf class_pred of the kept rows in descending score order; rows from
 *   min(count, max_det) on are zero.  count [B] = rows kept BEFORE the max_det cap (count > max_det: truncated).
 *   anchor_idx [B][max_det] (NULL = skip) = source anchor of each row, -1 past the last.
 *   Supported: 1 <= A <= 16384 anchors per image, 1 <= num_classes <= 80, 1 <= B <= 65535; anything else returns non-zero with
 *   the last error set before any launch.  Non-finite inputs are outside the contract but terminate in bounds.
 *   ws: the ws_bytes query's size (52 bytes per anchor and image; 0 = shape unsupported), contents need not survive the call. */
size_t rvt_yolox_postprocess_ws_bytes(int B, int A, int num_classes);
int rvt_yolox_postprocess(const float* pred, int B, int A, int num_classes, float conf_thre, float nms_thre, int class_agnostic,
                          int max_det, float* det, int* count, int* anchor_idx, void* ws, size_t ws_bytes, void* stream);

/* The eval-mode detection tail in ONE launch: head maps in, padded detections out (rvt_amd/csrc/nms.hpp, yolox_detect_kernel; host
 * mirror rvt_amd/postprocess.py: detect_padded).  Writes exactly what rvt_yolox_decode into pred_infer for every level followed by
 * rvt_yolox_postprocess writes, bit for bit, without the [B][A][5+nc] fp32 tensor between them.
 *   reg_obj[l] / cls[l] (HOST arrays of L device pointers, read during the call): level l's maps [B*H*W][ld_ro] and [B*H*W][ld_cls]
 *   of `dtype` (fp32 or bf16) as rvt_yolox_decode takes them; level_hw / level_stride as rvt_simota_loss takes them, 1 <= L <= 8,
 *   the levels must add up to A.  The level table and the pointers travel by value in the kernel arguments.
 *   Score: sigmoid of the objectness logit times the max over the SIGMOIDS of the class logits (lowest class on an exact tie of the
 *   sigmoid values), one fp32 multiply.  The box is decoded for the candidates only, with the decode kernel's expressions:
 *   (reg + grid) * stride for the centre, expf(reg) * stride for the extent.  conf_thre .. anchor_idx, the ordering rules, det /
 *   count / anchor_idx and the supported ranges are those of rvt_yolox_postprocess; more than 8 levels, a null map, ld_ro < 5 or
 *   ld_cls < num_classes also return non-zero with the last error set before any launch.  Allocates nothing, never synchronises:
 *   capturable.  ws: the ws_bytes query's size (the same 52 bytes per anchor and image), contents need not survive the call. */
size_t rvt_yolox_detect_ws_bytes(int B, int A, int num_classes);
int rvt_yolox_detect(const void* const* reg_obj, const void* const* cls, int ld_ro, int ld_cls, int dtype, const int* level_hw,
                     const int* level_stride, int L, int B, int A, int num_classes, float conf_thre, float nms_thre, int class_agnostic,
                     int max_det, float* det, int* count, int* anchor_idx, void* ws, size_t ws_bytes, void* stream);

/* Zero state rows of samples with mask[b] != 0 (modules/utils/detection.py:96-113).
 * st is [B][per_sample] of float32 (is_f32) or `dtype`. */
int rvt_state_reset_masked(void* st, const unsigned char* mask, int dtype, int B, size_t per_sample, void* stream);

/* Parameter-side tables (rvt_amd/csrc/pack.hpp; built by rvt_amd/weights.py).  One launch walks an array of descriptors in
 * DEVICE memory, 8-byte aligned; the pointers in a row are device pointers that outlive the launches (parameter storage,
 * packed-weight buffers, gradient buckets).  block0 of a row = the blocks of all rows before it (ascending, row 0 has 0).
 *   rvt_pack_table: element-wise gathers fp32 parameter -> kernel-side layout (cast, transpose with LayerScale folded in,
 *     tap-major conv weights, stride-parity conv-dgrad panels, gate-interleaved ConvLSTM rows) and the accumulating unpack
 *     of the raw conv weight gradient — what the reference leaves to autograd / .to() / permute (maxvit.py:51-53,160-168,
 *     rnn.py:52-61).  A row owns ceil(n / RVT_PACK_BLOCK_ELEMS) blocks; total_blocks = their sum.
 *   rvt_layerscale_grad_table: LayerScale (maxvit.py:51-53) folded out of the weight gradients of the proj / fc2 linears, whose
 *     input-gradient weights carry gamma: dW += gamma*S, db += gamma*cs, dgamma += rowsum(W*S) + b*cs.  A row owns C blocks
 *     (one per output channel); total_blocks = their sum. */
enum {                               /* RvtPackDesc.kind: element-wise gather from one fp32 source into one destination */
    RVT_PACK_COPY = 0,               /* dst[i] = src[i] */
    RVT_PACK_TRANSPOSE = 1,          /* src [R][K] -> dst [K][R], optionally * scale[r]      (d0 = R, d1 = K) */
    RVT_PACK_CONV_FWD = 2,           /* src [Cout][Cin][k][k] -> dst [Cout][k*k*cp] tap-major, cin fastest, zero padded (d0..d3 = Cout,Cin,k,cp) */
    RVT_PACK_CONV_DGRAD = 3,         /* src [Cout][Cin][k][k] -> dst [Cin][nky*nkx*Cout] of one stride-parity class (d0..d4 = Cout,Cin,k,nky,nkx) */
    RVT_PACK_LSTM_ROWS = 4,          /* src [4C][K] -> dst rows interleaved n' = (c/8)*32 + gate*8 + c%8            (d0 = C, d1 = K) */
    RVT_PACK_CONV_WGRAD_ACC = 5,     /* src [Cout][k*k*cp] (raw fp32 product) -> dst [Cout][Cin][k][k] += ...      (d0..d3 = Cout,Cin,k,cp) */
    RVT_PACK_CONV_DGRAD4 = 6         /* src [Cout][Cin][3][3] -> dst [(py,px,ci)][(da,db,co)] of the 2 x 2-block input gradient (ppgemm.hpp
                                        GATHER; d0, d1 = Cout, Cin): w[co][ci][ky][kx], ky = 1 | 2, 0 for py = 0 | 1 and da = 0, 1; else 0 */
};
enum { RVT_PACK_BLOCK_ELEMS = 1024 };    /* consecutive destination elements of one descriptor per logical block (what block0 counts) */
typedef struct RvtPackDesc {
    const float* src;
    void* dst;
    const float* scale;
    long long n;              /* destination elements */
    int kind;                 /* RVT_PACK_* */
    int out_f32;              /* destination is fp32 whatever the launch dtype */
    int d[5];
    int ky[4], kx[4];         /* RVT_PACK_CONV_DGRAD: the taps of the parity class */
    unsigned block0;          /* first block of this descriptor within the launch */
} RvtPackDesc;
typedef struct RvtLayerScaleDesc {
    const float* S; const float* cs;      /* raw products of the OUTER cotangent dy: S[c][k] = sum_tok dy[tok][c] a[tok][k],
                                             cs[c] = sum_tok dy[tok][c] */
    const float* W; const float* b; const float* gamma;
    float* dW; float* db; float* dgamma;  /* accumulated (+=) */
    int C, K;
    unsigned block0; int pad;
} RvtLayerScaleDesc;
int rvt_pack_table(const RvtPackDesc* descs, int n_desc, int total_blocks, int dtype, void* stream);
int rvt_layerscale_grad_table(const RvtLayerScaleDesc* descs, int n_desc, int total_blocks, void* stream);

/* Event stream -> stacked histogram, the uint8 event tensor the backbone consumes (data/utils/representations.py:76-117,
 * StackedHistogram.construct): x, y, pol (0/1), time are int64 [n_events], time sorted ascending.
 * out[(pol*bins + t_idx)][y][x] = min(count, count_cutoff) as uint8 [2*bins][H][W], with the reference's accumulator
 * wrap-around (uint8 if fastmode else int16).  scratch: 2*bins*H*W uint32 (zeroed here).  Bit-exact. */
int rvt_stacked_histogram(const long long* x, const long long* y, const long long* pol, const long long* time,
                          size_t n_events, int bins, int H, int W, int count_cutoff, int fastmode, unsigned* scratch,
                          unsigned char* out, void* stream);

/* Raw event streams -> a whole sequence of stacked-histogram windows (rvt_amd/csrc/evseq.hpp; host mirror
 * rvt_amd.representations.EventSequenceBuilder).  Replaces the window loop of scripts/genx/preprocess_dataset.py:480-534: two
 * searchsorted over the timestamps, one StackedHistogram.construct per window and, for the 1 Mpx sensor, the half-scale
 * nearest-exact interpolate of the full-size histogram.  Bit-exact with that composition for any event order.
 *
 * streams: B rows of RvtEventStream (below) in DEVICE memory, 8-byte aligned.  x, y, p are all of coord_bytes = 2 (int16), 4 (int32)
 *   or 8 (int64) bytes, one width per call; n is read on the device, so a captured graph replays after the host rewrote events
 *   and n in place, up to the buffers' capacity.
 * Window w of sample b:  end = searchsorted(t, ts_end[w], side='right');  window_us > 0: start = searchsorted(t, ts_end[w] -
 *   window_us, side='left');  window_events > 0: start = max(end - window_events, 0).  Exactly one of the two is positive.
 *   bounds int64 [B][T][2] receives (start, end).  Windows may overlap and may be empty (an all-zero image).
 * Per window, with t0 = t[start], t1 = t[end-1]:  t_idx = min(floorf((float)(t - t0) / (float)max(t1 - t0, 1) * bins), bins - 1)
 *   (fp32, correctly rounded, no contraction: the rule of the per-window entry above), polarity < 0 counts as 0, events with
 *   polarity > 1 or a coordinate outside the H x W sensor are skipped.  downsample_by_2: events with even x or even y are dropped
 *   and the rest counted at (y >> 1, x >> 1) of an H/2 x W/2 image, which IS interpolate(scale_factor=0.5, mode='nearest-exact')
 *   of the full-size histogram (source pixel 2i + 1), without ever forming it.  Then the accumulator wrap (uint8 if fastmode
 *   else int16 and clamp(min=0)) and min(count_cutoff), as above.
 * out uint8 [T][B][2*bins][H'][W'] (H' = H/2, W' = W/2 when down-sampling): window w of sample b at out + (w*B + b) * 2*bins*H'*W'.
 *   Any byte alignment; nothing outside those B*T images is written.
 * scratch: the ws_bytes query's size for windows_in_flight images of 32-bit counters, 16-byte aligned.  It must be ALL ZERO on entry
 *   and is left all zero (the narrowing pass clears what it has read: no memset per call).  The B*T windows go through in
 *   chunks of windows_in_flight: one count and one narrowing launch per chunk, after one launch for all bounds.
 * count_blocks: workgroups per window of the count launch (they stride over the window; the grid cannot depend on bounds that
 *   live on the device); 0 = sized by the library (about 2048 over a chunk, 8..256 per window). */
typedef struct RvtEventStream {
    const void* x;            /* n coordinates / polarities each */
    const void* y;
    const void* p;
    const long long* t;       /* n timestamps in microseconds, NON-DECREASING (rvt_event_time_repair / rvt_event_decode_dat below make them so) */
    long long n;
    const long long* ts_end;  /* the T window end timestamps of that sample (rows may share one array) */
} RvtEventStream;
size_t rvt_event_sequence_ws_bytes(int bins, int H, int W, int downsample_by_2, int windows_in_flight);
int rvt_event_sequence(const RvtEventStream* streams, int B, int T, int coord_bytes, long long window_us, long long window_events, int bins,
                       int H, int W, int downsample_by_2, int count_cutoff, int fastmode, long long* bounds, void* scratch,
                       int windows_in_flight, int count_blocks, unsigned char* out, void* stream);

/* What comes before the event stream (rvt_amd/csrc/evprep.hpp; host mirrors rvt_amd.representations.repair_time and
 * rvt_amd.recordings.DatDecoder): the reference reader's timestamp repair (scripts/genx/preprocess_dataset.py:163-172, _correct_time)
 * and the decode of packed Prophesee Event2D records (utils/evaluation/prophesee/io/dat_events_tools.py:41-50, load_td_data).
 * rvt_event_sequence keeps its precondition (t non-decreasing); these entries are what establishes it.  Integer work: bit-exact.
 *
 * Repair: t_out[i] = max(c, t[0], ..., t[i]) over the n timestamps of a row, c = carry[b] when carry is non-null, else 0 (the
 *   reference starts at 0, so negative timestamps become 0).  With carry, carry[b] = max(c, every t) afterwards: a producer that
 *   delivers a stream in chunks gets exactly the repair of the concatenated stream.  carry int64 [B].
 * Two launches, grid (blocks_per_stream, B), each workgroup one contiguous span of its stream; no workgroup waits for another.
 *   The first reduces the spans to maxima in ws and parks the carry-in there (the only reader of carry), the second scans and
 *   writes carry (its only writer).  blocks_per_stream 0..4096, 0 = sized by the library; ws: rvt_event_prep_ws_bytes(B,
 *   blocks_per_stream) bytes, 8-byte aligned, any contents; with K = that size / (8 * B) - 1 workgroups per stream,
 *   repaired (optional) int64 [B][K]: workgroup k of stream b WRITES the number of timestamps it changed into [b][k].
 * rvt_event_time_repair: in place on the t arrays of the B rows (n read on the device); only changed timestamps are stored.
 * rvt_event_decode_dat: records = DEVICE array of B device pointers to packed records {uint32 t; int32 w}, each 8-byte aligned;
 *   n_records int64 [B] on the device.  n = min(n_records[b], capacity) records are decoded from index 0 into the x, y, p, t
 *   arrays row b points at (coord_bytes = 2, 4 or 8 for x, y, p) and n is written into row b: x = w & 16383, y = (w >> 14) & 16383,
 *   p = (w >> 28) & 1, t zero-extended.  Nothing behind index n is written.  A captured graph replays after the host rewrote
 *   records and n_records in place.  repair != 0: the timestamps are repaired in the same pass (records read twice, stream
 *   written once); repair == 0: one launch, carry and ws are not touched (ws may be null).  16-byte accesses where a base is 16-byte aligned. */
size_t rvt_event_prep_ws_bytes(int B, int blocks_per_stream);
int rvt_event_time_repair(const RvtEventStream* streams, int B, long long* carry, long long* repaired, void* ws, int blocks_per_stream,
                          void* stream);
int rvt_event_decode_dat(const void* const* records, const long long* n_records, long long capacity, RvtEventStream* streams, int B,
                         int coord_bytes, int repair, long long* carry, long long* repaired, void* ws, int blocks_per_stream, void* stream);

/* The reference's second representation, MixedDensityEventStack (data/utils/representations.py:130-218, selected by
 * scripts/genx/conf_preprocess/representation/mixeddensity_stack.yaml, built in scripts/genx/preprocess_dataset.py:663-679), on the
 * kernels of the sequence entry above (rvt_amd/csrc/evseq.hpp; host mirrors rvt_amd.representations.MixedDensityEventStack and
 * EventSequenceBuilder(representation='mixed_density')).  Per window, with t0 / t1 its first / last timestamp:
 *     tn  = clamp((float)(t - t0) / (float)max(t1 - t0, 1), 1e-6f, (float)(1 - 1e-6))        (fp32, one correctly rounded division)
 *     bin = max(bins + e, 0), e = the unbiased binary exponent of tn = floor(log2(tn))         (representations.py:205-208)
 *     img[bin][y][x] += polarity ? +1 : -1;   out[b] = int8(sum of img[0..b]) (low 8 bits, two's complement: the reference's int8
 *     accumulator wrap and the wrap of its cumsum_channel);   count_cutoff >= 0: clamp to [-count_cutoff, count_cutoff] (<= 127);
 *     count_cutoff < 0: no clamp.
 *   The exponent IS the floor of the reference's bins - log(tn) / log(1/2).  The reference evaluates that quotient in fp32; it
 *   agrees with the exponent for every event of a window whose span t1 - t0 is at most 2^20 us (every duration the reference ships
 *   is 50 ms), so the output is bit-identical there.  On longer windows the reference itself puts an event whose tn lies a few
 *   ulps below a power of two one bin too high (span 2^24, offset 8388606: reference bin 9 of 10, exact bin 8); this library
 *   returns the exact bin.  Polarity < 0 counts as 0; events with polarity > 1 or a coordinate outside the sensor are skipped.
 *
 * rvt_mixed_density_stack: one window; x, y, pol, time int64 [n_events], time non-decreasing (MixedDensityEventStack.construct).
 *   out int8 [bins][H][W], any byte alignment.  scratch: bins*H*W int32, 16-byte aligned, ALL ZERO on entry and left all zero.
 * rvt_event_sequence_mixed: the arguments, stream table, window rule, bounds, chunking and scratch contract of rvt_event_sequence
 *   (no fastmode), scratch sized by rvt_event_sequence_mixed_ws_bytes (half the histogram's: bins planes, not 2*bins).
 *   downsample_by_2 is downsample_ev_repr (preprocess_dataset.py:467-477: +128, nearest-exact at half scale, -128), i.e. the odd
 *   pixels of the full-size stack; sum, wrap and clamp are per pixel and commute with that selection.
 *   out int8 [T][B][bins][H'][W']: window w of sample b at out + (w*B + b) * bins*H'*W'; nothing else is written. */
int rvt_mixed_density_stack(const long long* x, const long long* y, const long long* pol, const long long* time, size_t n_events,
                            int bins, int H, int W, int count_cutoff, int* scratch, signed char* out, void* stream);
size_t rvt_event_sequence_mixed_ws_bytes(int bins, int H, int W, int downsample_by_2, int windows_in_flight);
int rvt_event_sequence_mixed(const RvtEventStream* streams, int B, int T, int coord_bytes, long long window_us, long long window_events, int bins,
                             int H, int W, int downsample_by_2, int count_cutoff, long long* bounds, void* scratch,
                             int windows_in_flight, int count_blocks, signed char* out, void* stream);

/* Spatial training augmentation (rvt_amd/csrc/augment.hpp; data/utils/augmentor.py RandomSpatialAugmentorGenX and
 * data/genx_utils/labels.py): horizontal flip, then zoom-in or zoom-out, of a batch of sequences and of their box labels.
 * Frame f belongs to sample f % B; every per-sample parameter is read from a device table the host writes, so neither call
 * synchronises with the host and both replay in a hipGraph with a rewritten table.  Bit-exact with the reference.
 *
 * rvt_augment_planes: in / out uint8 [F][C][H][W] (the loader's NCHW planes), out must not overlap in.  A list of T separately
 *   allocated (B,C,H,W) tensors is one call per tensor with F = B.  table int32 [B][8]: flip, mode (0 none, 1 zoom-in,
 *   2 zoom-out), x0, y0, zh, zw, 0, 0 with zh = int(H / factor), zw = int(W / factor) computed by the host in double.
 *     n(i; n_out, n_in) = min((int)floorf((i + 0.5f) * ((float)n_in / (float)n_out)), n_in - 1)     (PyTorch's nearest-exact)
 *     S[y][x] = flip ? in[y][W-1-x] : in[y][x]
 *     mode 0: out = S;   mode 1: out[y][x] = S[y0 + n(y; H, zh)][x0 + n(x; W, zw)];
 *     mode 2: out[y][x] = S[n(y-y0; zh, H)][n(x-x0; zw, W)] for y0 <= y < y0+zh and x0 <= x < x0+zw, else 0.
 *   The kernel clamps the window into the frame, so any table contents terminate in bounds; a window outside the frame is the
 *   host's to reject.  16-byte accesses when W % 16 == 0 and both bases are 16-byte aligned, byte accesses otherwise.
 *   Supported: 1 <= W <= 2048, C*H <= 2^24; anything else returns non-zero with the last error set before any launch.
 *
 * rvt_augment_labels: rows fp32 [F][G][7] (t x y w h class_id class_confidence), count int32 [F] (-1 = a frame without
 *   labels).  rows_out [F][G][7]: the surviving rows in their original order, zero rows behind them; count_out [F]: survivors,
 *   -1 carried through; yolox_out [F][G][5] (NULL = skip): class, x + 0.5*w, y + 0.5*h, w, h of the survivors, zero padded.
 *   table fp32 [B][12]: flip, mode, W-1, x0, y0, hx, hy, m, capx, capy, 0, 0 (each computed in double and rounded once).
 *   Every line is one rounded fp32 operation, no fused multiply-add:
 *     flip:     x = ((W-1) - x) - w
 *     mode 1:   cx0 = min(max(x, x0), hx); cx1 = min(max(x + w, x0), hx) (y likewise); x = cx0 - x0; w = cx1 - cx0;
 *               rows without w > 0 and h > 0 are dropped; then scale
 *     mode 2:   scale; then x = x + x0; y = y + y0
 *     scale:    x1 = min((x + w) * m, capx); y1 likewise; x = x * m; y = y * m; w = x1 - x; h = y1 - y; dropped unless w, h > 0
 *   with, for zoom factor f:  mode 1: hx = min(x0 + W/f, W-1) - 1, m = f, capx = f * (W/f) - 1;  mode 2: m = 1/f,
 *   capx = (1/f) * W - 1 (y likewise). */
enum { RVT_AUGMENT_PLANES_COLS = 8, RVT_AUGMENT_LABEL_COLS = 12 };    /* entries of one sample's row of the two tables */
int rvt_augment_planes(const void* in, void* out, const int* table, int F, int B, int C, int H, int W, void* stream);
int rvt_augment_labels(const float* rows, const int* count, const float* table, int F, int B, int G, float* rows_out, int* count_out,
                       float* yolox_out, void* stream);

/* Sparse frame cache (rvt_amd/csrc/framecache.hpp; host mirror rvt_amd/framecache.py): a lossless codec for byte planes that are
 * mostly zero, the device counterpart of the reference's compressed pre-processed store (data/genx_utils/sequence_base.py:92-102).
 * Built event tensors are kept as a bitmap plus their non-zero bytes and fetched back by frame index.  Integer work: bit-exact.
 *
 * Format, version 1.  A frame is E bytes (uint8, or int8 seen as uint8), 1 <= E < 2^31, a multiple of nothing; a packed set holds F
 * frames of one E.  A group is 64 consecutive bytes of a frame, Gf = ceil(E / 64); a segment is 64 consecutive groups (4096
 * bytes), Sf = ceil(Gf / 64).
 *   masks      uint64 [F][Gf]      bit i of group g is set iff byte 64 g + i of the frame exists and is non-zero (the bits of the last
 *                                  group beyond E are 0)
 *   seg_offset uint32 [F][Sf + 1]  exclusive prefix sum of the per-segment non-zero counts of the frame; the last entry is the frame's count
 *   value_base int64  [F + 1]      exclusive prefix sum of the frames' counts; value_base[F] is the total, nnz
 *   values     uint8  [capacity]   the non-zero bytes of all frames, frame order then byte order, no padding
 *   status     int32  [1]          bit 0: pack / gather ran out of capacity;  bit 1: unpack met an index outside [-1, F);
 *                                  bit 2: gather met a table row whose count is outside [0, E]
 * Packed size: 8 Gf F + 4 (Sf + 1) F + 8 (F + 1) + nnz bytes.
 *
 * rvt_frames_pack: frames [F][E] -> masks, seg_offset, value_base, values, status.  Four launches on the stream (masks + counts,
 *   the two prefix sums, value compaction; three when capacity is 0), no host synchronisation, no allocation; ws:
 *   rvt_frames_pack_ws_bytes(F, E) bytes (0 = F or E out of range), 4-byte aligned, any contents.  status is WRITTEN: 1 when
 *   nnz > capacity, else 0.  Out of capacity, masks, seg_offset and value_base are still complete (value_base[F] is the room a retry
 *   needs) and exactly the value bytes below `capacity` are written.  Nothing behind values[min(nnz, capacity)] is written, and a
 *   run's first and last bytes leave by byte stores: memory next to the run is never read and rewritten.  16-byte loads when a frame
 *   starts on a 16-byte boundary (frames aligned and E % 16 == 0), byte loads otherwise.
 * rvt_frames_unpack: out [Fout][E], frame i = frame index[i] of the packed set (index int64 [Fout] on the device; NULL = frames
 *   0 .. Fout-1 in order).  index -1 writes a zero frame (the padded tail of a stream); any other index outside [0, F) writes a zero
 *   frame and ORS bit 1 into status (nothing else touches status: clear it before the call to read it afterwards).  One launch, no
 *   workspace; replays in a hipGraph after the packed arrays and the index were rewritten in place.  Reads of values stay inside
 *   [0, values_len) whatever the arrays hold; out is written as whole aligned 16-byte lines with byte stores only at the ends of a
 *   4096-byte segment that does not start or end on one, so out may sit at any byte address and nothing outside out[Fout][E] is
 *   written.  masks / value_base / index 8-byte, seg_offset / status 4-byte aligned.
 * rvt_frames_unpack_augment: out [Fout][C][H][W] = rvt_augment_planes(rvt_frames_unpack(..., index), table), bit for bit, in one
 *   launch and without the dense tensor between the two (rvt_amd/csrc/frames_augment.hpp).  E must equal C*H*W.  Output frame i is
 *   packed frame index[i] (NULL = frame i) transformed by table row i % B; the table is rvt_augment_planes' int32 [B][8] (flip,
 *   mode, x0, y0, zh, zw, 0, 0) and is clamped into the frame in the same way.  index -1 writes a zero frame whatever the table
 *   says; any other index outside [0, F) writes a zero frame and ORS bit 1 into status.  Several output frames may name one packed
 *   frame under different table rows.  Bytes are moved, never interpreted (an int8 store works as uint8).  One launch, no workspace,
 *   no allocation, no host synchronisation; replays in a hipGraph after index, table and the packed arrays were rewritten in
 *   place.  Reads of values stay inside [0, values_len) and mask bits behind a frame's end are ignored whatever the arrays hold;
 *   nothing outside out[Fout][E] is written.  16-byte stores when W % 16 == 0 and out is 16-byte aligned, byte accesses otherwise.
 *   Supported: 1 <= W <= 2048, C*H <= 2^24; masks / value_base / index 8-byte, seg_offset / status / table 4-byte aligned.
 * rvt_frames_gather: n frames named by address, out of any number of packed sets of one E, into the packed set masks [n][Gf],
 *   seg_offset [n][Sf + 1], value_base [n + 1], values [capacity] on the device (rvt_amd/csrc/frames_gather.hpp): bit for bit the
 *   concatenation of the single-frame slices in table order.  table: int64 [n][4] in DEVICE memory, 8-byte aligned, row f =
 *   {address of the frame's Gf masks (8-byte aligned), address of its Sf + 1 seg_offset entries (4-byte aligned), address of its
 *   first value byte (any; may be 0 when the count is 0), its count of non-zero bytes}.  The addresses may point into memory of the
 *   same device or into PINNED host memory (never pageable memory); rows may name any mix of sets in any order and one frame twice.
 *   value_base is the exclusive prefix sum of the counts, made on the device; values are back to back.  status is WRITTEN: bit 0
 *   when the total exceeds capacity (value_base is still complete and exactly the value bytes below capacity are written), bit 2
 *   when a row's count was outside [0, E] (it is taken as 0).  Nothing outside values[0, min(total, capacity)) and the n rows of
 *   the three other arrays (n + 1 entries of value_base) is written; the first and last bytes of a frame's values leave by byte
 *   stores (memory beside a run is never read and rewritten) and no byte outside a frame's masks, seg_offset row and count value
 *   bytes is read.  Two launches on the stream (the prefix sum, then the copy on at most max_blocks workgroups, 0 = the default,
 *   walked in fixed-size pieces), no workspace, no allocation, no host synchronisation, no workgroup waits for another; replays in
 *   a hipGraph after the table was rewritten in place.  n = 0 returns 0 and launches nothing.  masks / value_base 8-byte,
 *   seg_offset / status 4-byte aligned; values at any byte address. */
enum {                               /* the bits of status */
    RVT_FRAMES_STATUS_CAPACITY = 1,  /* bit 0 */
    RVT_FRAMES_STATUS_INDEX = 2,     /* bit 1 */
    RVT_FRAMES_STATUS_COUNT = 4      /* bit 2 */
};
enum { RVT_FRAMES_GATHER_COLS = 4 };     /* int64 columns of a row of rvt_frames_gather's table */
size_t rvt_frames_pack_ws_bytes(long long F, long long E);
int rvt_frames_pack(const void* frames, long long F, long long E, void* masks, void* seg_offset, void* value_base, void* values,
                    long long capacity, void* status, void* ws, size_t ws_bytes, void* stream);
int rvt_frames_unpack(const void* masks, const void* seg_offset, const void* value_base, const void* values, long long values_len,
                      long long F, long long E, const long long* index, long long Fout, void* out, void* status, void* stream);
int rvt_frames_unpack_augment(const void* masks, const void* seg_offset, const void* value_base, const void* values,
                              long long values_len, long long F, long long E, const long long* index, long long Fout,
                              const int* table, int B, int C, int H, int W, void* out, void* status, void* stream);
int rvt_frames_gather(const long long* table, long long n, long long E, void* masks, void* seg_offset, void* value_base, void* values,
                      long long capacity, void* status, int max_blocks, void* stream);

/* Format, version 2 (rvt_amd/csrc/capi_frames2.hip; host mirror rvt_amd/framecache.py, PackedFrames2): version 1 with a second mask
 * level.  A mask word is kept only for the groups that hold a non-zero byte, so the fixed cost of a frame falls from 8 Gf bytes to
 * 16 Sf + 16 and the variable cost is 8 bytes per non-empty group.  Geometry (E, group, Gf, segment, Sf) as in version 1.
 *   group_mask uint64 [F][Sf]          bit g of segment s is set iff group 64 s + g exists and holds a non-zero byte
 *   seg_offset uint32 [F][Sf + 1]      as in version 1: exclusive prefix sum of the segments' non-zero byte counts, last entry = the frame's count
 *   grp_offset uint32 [F][Sf + 1]      exclusive prefix sum of popcount(group_mask[f][s]), last entry = the frame's count of non-empty groups
 *   value_base int64  [F + 1]          as in version 1
 *   mask_base  int64  [F + 1]          exclusive prefix sum of the frames' non-empty group counts; mask_base[F] = ngroups
 *   masks      uint64 [mask_capacity]  version 1's mask of each NON-EMPTY group, frame order then group order, no padding; the bits
 *                                      behind E are zero; no stored word is zero
 *   values     uint8  [capacity]       as in version 1
 *   status     int32  [1]              the version-1 bits; bit 0: nnz > capacity or ngroups > mask_capacity
 * The mask of group g (segment s, bit j) is masks[mask_base[f] + grp_offset[f][s] + popcount(group_mask[f][s] & ((1 << j) - 1))] when
 * bit j of group_mask[f][s] is set, and 0 otherwise.
 * Packed size, status excluded: 16 Sf F + 8 F + 16 (F + 1) + 8 ngroups + nnz bytes.
 *
 * rvt_frames_pack2: frames [F][E] -> the seven arrays and status.  Four launches on the stream (group masks + counts, the prefix
 *   sums per frame, the prefix sums over the frames, compaction of masks and values; three when both capacities are 0), no host
 *   synchronisation, no allocation; ws: rvt_frames_pack2_ws_bytes(F, E) bytes (0 = F or E out of range), 4-byte aligned, any
 *   contents.  status is WRITTEN: 1 when nnz > capacity or ngroups > mask_capacity, else 0.  Out of capacity, the five index arrays
 *   are still complete (value_base[F] and mask_base[F] are the room a retry needs) and exactly the value bytes below `capacity` and
 *   the mask words below `mask_capacity` are written: nothing behind either, mask words by aligned 8-byte stores, a value run's
 *   first and last bytes by byte stores (memory next to a run is never read and rewritten).
 * rvt_frames_unpack2: out [Fout][E] by index, with rvt_frames_unpack's rules: index NULL = frames 0 .. Fout-1, -1 writes a zero
 *   frame, any other index outside [0, F) writes a zero frame and ORS bit 1 into status.  One launch, no workspace; replays in a
 *   hipGraph after the packed arrays and the index were rewritten in place.  Reads of masks stay inside [0, masks_len) and reads of
 *   values inside [0, values_len) whatever the other arrays hold; a segment whose group_mask word is 0 loads no mask and no value.
 *   out may sit at any byte address and nothing outside out[Fout][E] is written.
 * rvt_frames_gather2: rvt_frames_gather for version-2 sets: bit for bit the concatenation of the single-frame slices in table order.
 *   table: int64 [n][8] in DEVICE memory, row f = {address of the frame's Sf group_mask words (8-byte aligned), address of its Sf + 1
 *   seg_offset entries, address of its Sf + 1 grp_offset entries (4-byte aligned), address of its first compacted mask (8-byte
 *   aligned; may be 0 when the group count is 0), address of its first value byte (any; may be 0 when the count is 0), its count of
 *   non-zero bytes, its count of non-empty groups, 0}; device or PINNED host addresses.  value_base and mask_base are made on the
 *   device.  status is WRITTEN: bit 0 when the value total exceeds capacity or the group total mask_capacity (the five index arrays
 *   are still complete and exactly the entries below the capacities are written), bit 2 when a row's value count was outside
 *   [0, E] or its group count outside [0, Gf] (it is taken as 0).  Two launches (the prefix sums, then the copy on at most
 *   max_blocks workgroups, 0 = the default), no workspace, no allocation, no host synchronisation; replays in a hipGraph after the
 *   table was rewritten in place.  n = 0 returns 0 and launches nothing.
 * All three: group_mask / value_base / mask_base / masks / index / table 8-byte, seg_offset / grp_offset / status 4-byte aligned. */
enum { RVT_FRAMES_GATHER2_COLS = 8 };    /* int64 columns of a row of rvt_frames_gather2's table */
size_t rvt_frames_pack2_ws_bytes(long long F, long long E);
int rvt_frames_pack2(const void* frames, long long F, long long E, void* group_mask, void* seg_offset, void* grp_offset, void* value_base,
                     void* mask_base, void* masks, long long mask_capacity, void* values, long long capacity, void* status, void* ws,
                     size_t ws_bytes, void* stream);
int rvt_frames_unpack2(const void* group_mask, const void* seg_offset, const void* grp_offset, const void* value_base,
                       const void* mask_base, const void* masks, long long masks_len, const void* values, long long values_len,
                       long long F, long long E, const long long* index, long long Fout, void* out, void* status, void* stream);
int rvt_frames_gather2(const long long* table, long long n, long long E, void* group_mask, void* seg_offset, void* grp_offset,
                       void* value_base, void* mask_base, void* masks, long long mask_capacity, void* values, long long capacity,
                       void* status, int max_blocks, void* stream);

/* Detection previews (rvt_amd/csrc/capi_viz.hip; host mirror rvt_amd/viz.py): event planes and box lists to RGB images, the device
 * counterpart of the reference's detection visualisation callback (callbacks/viz_base.py:164-174 ev_repr_to_img, callbacks/detection.py:
 * 52-62, utils/evaluation/prophesee/visualize/vis_utils.py:88-106).  Integer work: bit-exact.  Everything below is defined at the
 * resolution of the planes (H x W); `scale` s in {1, 2, 4} replicates the finished image: output pixel (Y, X) is base pixel
 * (Y / s, X / s), Hs = H s, Ws = W s.
 *
 * rvt_render_preview: planes [F][C][H][W], uint8 or (planes_signed != 0) int8, C even, 2 <= C <= 512, H, W <= 2^20.
 *   Base image: d = (sum of channels C/2 .. C-1) - (sum of channels 0 .. C/2-1) in int32; d > 0 -> (255, 255, 255), d < 0 ->
 *   (0, 0, 0), d == 0 -> (127, 127, 127): the reference's ev_repr_to_img, its reading of the first half as "negative" included.
 *   Panels: P = 1 or 2, all on the same base image, panel p with its own box list or none (rows NULL): rows fp32 [F][N][7],
 *   count int32 [F], kind.  RVT_VIZ_KIND_DET: the detection row of the post-processing entry (x1 y1 x2 y2 obj class_conf class):
 *   x = x1, y = y1, w = x2 - x1, h = y2 - y1 (one rounded fp32 subtraction each), score = class_conf.  RVT_VIZ_KIND_LABEL: the
 *   label row of the augmentation entry (t x y w h class_id conf).  A frame draws its first n = clamp(count[f], 0, min(N,
 *   RVT_VIZ_MAX_BOXES)) rows (a label count of -1: none); rows behind RVT_VIZ_MAX_BOXES are not drawn.
 *   One box: x0 = trunc(x), y0 = trunc(y), x1 = x0 + trunc(w), y1 = y0 + trunc(h), cls = trunc(class), truncation toward zero.
 *   Skipped when any of x, y, w, h, class is not finite or of magnitude >= 2^20, or w < 0, h < 0 or class < 0.  Outline: the
 *   pixels inside the image with (x0 <= x <= x1 and y in {y0, y1}) or (y0 <= y <= y1 and x in {x0, x1}), colour
 *   palette[cls % n_palette] (palette uint8 [n_palette][3], device).
 *   Tag (flags & RVT_VIZ_TEXT): the text is names[cls % n_names] (names uint8 [n_names][RVT_VIZ_NAME_BYTES], zero-terminated
 *   ASCII or all 12 bytes; n_names <= 4096), for a detection followed by ' ' and the score as d.dd with the digits of
 *   q = (int)(score * 100.0f + 0.5f) clamped to [0, 100] (one fp32 multiply, one fp32 add, a truncation; a score that is not
 *   finite prints 1.00 for +inf and 0.00 otherwise).  A filled rectangle in the box colour, 6 len + 1 wide and 9 high, left edge
 *   x0, top ty = y0 - 9 when that is >= 0, else y0 + 1, clipped to the image.  Character i sits in the 6 x 8 cell whose top left
 *   pixel is (x0 + 1 + 6 i, ty + 1): bit 4 - gx of glyphs[ch & 127][gy] lights pixel (gx, gy) of the cell, gx < 5, gy < 7
 *   (glyphs uint8 [128][RVT_VIZ_GLYPH_ROWS], device).  Glyph pixels are black when r + g + b >= 384, white otherwise.
 *   Order: painter's, in row order: the base image, then for j = 0 .. n-1 the outline of box j, then its tag.
 *   out uint8 [Fout][P][Hs][Ws][3]; seen as [Fout][P Hs][Ws][3] it is the reference's prediction-over-label stack.  Image i
 *   shows frame f = frame_index[i] (int64 [Fout] on the device; NULL: f = i, and Fout <= F), box lists indexed by f.  f == -1
 *   writes an all-zero image; any other f outside [0, F) writes an all-zero image and ORS RVT_VIZ_STATUS_INDEX into status
 *   (int32 [1]; nothing else touches it: clear it before the call to read it afterwards).
 *   One launch for all images and panels: no workspace, no allocation, no host synchronisation, no atomics; replays in a hipGraph
 *   after planes, rows, counts and frame_index were rewritten in place.  The planes of a frame are read once for all panels; every
 *   byte of out is written exactly once and none is read; nothing outside out[Fout][P][Hs][Ws][3] is written, at any byte address
 *   of out.  16-byte loads and stores when W % 16 == 0 and planes and out are 16-byte aligned, byte accesses through the same
 *   code otherwise.  rows / count / status 4-byte, frame_index 8-byte aligned.  Anything unsupported returns non-zero with the
 *   last error set before any launch. */
enum { RVT_VIZ_KIND_DET = 0, RVT_VIZ_KIND_LABEL = 1 };
enum { RVT_VIZ_TEXT = 1 };               /* flags */
enum { RVT_VIZ_STATUS_INDEX = 1 };       /* the bit of status */
enum { RVT_VIZ_MAX_BOXES = 512, RVT_VIZ_NAME_BYTES = 12, RVT_VIZ_GLYPH_ROWS = 7 };
int rvt_render_preview(const void* planes, int planes_signed, long long F, int C, int H, int W, const float* rows0, const int* count0,
                       int N0, int kind0, const float* rows1, const int* count1, int N1, int kind1, int P, const long long* frame_index,
                       long long Fout, const unsigned char* palette, int n_palette, const unsigned char* names, int n_names,
                       const unsigned char* glyphs, int scale, int flags, void* out, int* status, void* stream);

/* The optimizer step on the device (rvt_amd/csrc/optim.hpp; host mirror rvt_amd/optim.py): gradient clipping by value, AdamW
 * (decoupled weight decay, no amsgrad) and the OneCycle learning-rate schedule of every parameter of every parameter group in one
 * call (reference modules/detection.py:360-392 and the trainer's gradient_clip_val by value).  Two tables in DEVICE memory, built
 * once by the host, 8-byte aligned:
 *   chunks [n_chunks] of RvtOptimChunk, one per piece of at most RVT_OPTIM_CHUNK_ELEMS consecutive elements of one parameter
 *     (fp32, contiguous): pieces of one tensor start that many elements apart; a shorter tensor is one entry.  A chunk whose
 *     four pointers are 16-byte aligned moves in 16-byte accesses, any other element by element.
 *   groups [n_groups] of RvtOptimGroup, all double like the Python floats torch keeps them in.
 *   step: int64 on the device, the optimizer steps done so far.  The call uses k = *step + 1 in every workgroup and leaves
 *     *step = k behind (a trailing one-thread launch of the same call), so a captured graph replays with nothing written by the host.
 * In double, per workgroup:  pos = k - 1;  lr = (lr_max - lr_init) * (pos / warm_end) + lr_init for pos <= warm_end,
 *   (lr_final - lr_max) * ((pos - warm_end) / (last - warm_end)) + lr_max for pos <= last, lr_final beyond (torch's OneCycleLR,
 *   three_phase=False, linear, raises there);  bc1 = 1 - beta1^k;  bc2 = 1 - beta2^k.
 * In fp32, per element, one rounded operation each (the constants computed in double and rounded once):
 *     g = clamp(g, -clip, clip)   (the stored gradient is NOT modified, unlike clip_grad_value_)
 *     p = p * (1 - lr * weight_decay);  m = m + (1 - beta1) * (g - m);  v = beta2 * v + ((1 - beta2) * g) * g
 *     p = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
 * max_blocks: grid cap, 0 = the default (2048 workgroups; chunks beyond are walked grid-stride). */
enum { RVT_OPTIM_CHUNK_ELEMS = 4096 };
typedef struct RvtOptimChunk {
    float* p;
    const float* g;
    float* m;                 /* exp_avg */
    float* v;                 /* exp_avg_sq */
    int n;                    /* 1 .. RVT_OPTIM_CHUNK_ELEMS elements */
    int group;                /* 0 .. n_groups - 1 */
} RvtOptimChunk;
typedef struct RvtOptimGroup {
    double beta1, beta2, eps, weight_decay;
    double clip;              /* < 0: no clipping */
    double lr_init, lr_max, lr_final;
    double warm_end;          /* end of the first phase as a schedule position: float(pct_start * total_steps) - 1, may be fractional */
    double last;              /* last position of the schedule: total_steps - 1.  No schedule: lr_init = lr_max = lr_final, 0, 0 */
} RvtOptimGroup;
int rvt_optim_step(const RvtOptimChunk* chunks, int n_chunks, const RvtOptimGroup* groups, int n_groups, long long* step, int max_blocks,
                   void* stream);

/* Gradient statistics and the non-finite guard on the device (rvt_amd/csrc/gradstats.hpp; host mirror rvt_amd/optim.py: GradMonitor;
 * reference callbacks/gradflow.py `GradFlowLogCallback` and the GradScaler step-skip of `precision: 16`).  rvt_grad_stats reduces the
 * fp32 gradient and parameter pieces of the optimizer's own chunk table: two launches, no host synchronisation, no allocation,
 * no floating-point atomics; the result is bit-reproducible and does not depend on max_blocks.
 *   Partial pass: workgroups stride over the chunks (max_blocks as in rvt_optim_step).  A chunk whose g and p are 16-byte aligned
 *     moves in 16-byte loads, any other element by element.  An element is NON-FINITE when (bits & 0x7f800000) == 0x7f800000.  Over
 *     the finite gradient elements, in double: sum |g|, sum g^2; in float: max |g|; int32 count of the non-finite ones.  sum p^2 in
 *     double runs over the finite PARAMETER elements (a parameter's norm does not depend on its gradient).  One RvtGradStat per
 *     chunk into ws (rvt_grad_stats_ws_bytes(n_chunks) bytes, 8-byte aligned, the caller's).
 *   Fold pass: one workgroup.  tensor_first: int32 [n_tensors + 1] on the device, tensor t owns the chunks tensor_first[t] ..
 *     tensor_first[t + 1] - 1 (consecutive in the table; an empty range gives a row of zeros with nonfinite = -1).  The rows of the
 *     tensors go to stats[slot * stat_stride + t], the totals to heads[slot], slot = *step % ring with *step the optimizer's device
 *     counter READ ON THE DEVICE (the call does not change it): a replayed graph fills slot after slot by itself.
 *   scalars: HOST array of n_scalars <= RVT_GRADSTAT_MAX_SCALARS device pointers to fp32 values (loss terms, ...), read by the call;
 *     the values they point to are read by the launch and copied into the slot's head.  NULL with n_scalars = 0.
 *   verdict: long long [2] on the device.  verdict[0] = the non-finite total of the latest observation (written here);
 *     verdict[1] = steps skipped so far (written by rvt_optim_step_guarded only).
 * rvt_optim_step_guarded is rvt_optim_step, bit for bit, when verdict[0] == 0.  Otherwise no p, m or v is written, *step stays, and
 * the trailing one-thread launch adds 1 to verdict[1]: a skipped step advances neither the bias correction nor the schedule. */
enum { RVT_GRADSTAT_MAX_SCALARS = 8 };
typedef struct {
    double abs_sum;           /* sum |g| over the finite gradient elements */
    double sq_sum;            /* sum g^2 over the finite gradient elements */
    double param_sq_sum;      /* sum p^2 over the finite parameter elements */
    float abs_max;            /* max |g| over the finite gradient elements, 0 when there is none */
    int nonfinite;            /* inf / NaN gradient elements; -1: the tensor had no chunk in this observation */
} RvtGradStat;
typedef struct {
    long long step;           /* *step at the observation = optimizer steps done before it */
    long long nonfinite;      /* total over the tensors */
    double sq_sum;            /* total over the tensors, in tensor order */
    float abs_max;            /* over the tensors */
    int n_scalars;
    float scalars[8];         /* RVT_GRADSTAT_MAX_SCALARS; the entries from n_scalars on are 0 */
} RvtGradStatHead;
size_t rvt_grad_stats_ws_bytes(int n_chunks);
int rvt_grad_stats(const RvtOptimChunk* chunks, int n_chunks, const int* tensor_first, int n_tensors, const long long* step,
                   const float* const* scalars, int n_scalars, RvtGradStat* stats, int stat_stride, RvtGradStatHead* heads, int ring,
                   long long* verdict, void* ws, size_t ws_bytes, int max_blocks, void* stream);
int rvt_optim_step_guarded(const RvtOptimChunk* chunks, int n_chunks, const RvtOptimGroup* groups, int n_groups, long long* step,
                           long long* verdict, int max_blocks, void* stream);

/* Prophesee / COCO mAP evaluation of detections on the device (rvt_amd/csrc/cocoeval.hpp; host mirror rvt_amd/evaluation.py).
 * Replaces utils/evaluation/prophesee/ (filter_boxes, evaluate_list, coco_eval.py) and the COCOeval core it calls (evaluateImg,
 * accumulate; bbox mode, iscrowd false, maxDets 100; the recall table also at maxDets 1 and 10): no per-frame copy to the host, no
 * Python loop.  No call synchronises with the host; all replay in a hipGraph.
 *
 * The match entry: one launch for F frames, one wave per (frame, category).
 *   det [F][max_det][7] fp32 and count [F] int32 exactly as the post-processing entry returns them (x1 y1 x2 y2 obj class_conf
 *   class_pred; det_xywh != 0: columns 0..3 are x y w h).  A frame uses its first min(count, max_det) rows; count > max_det adds
 *   one to the truncated-frames counter.  labels [F][G][7] fp32 (t x y w h class_id class_confidence) and label_count [F] int32
 *   (<= 0: no labels) as the label augmentation entry lays them out; t_us [F] int64, the frame's timestamp in microseconds.
 *   Filter (fp32, no fused multiply-add), for labels and detections alike: a box stays iff t_us > 500000 and
 *   w*w + h*h >= min_diag*min_diag and w >= min_side and h >= min_side; a detection's w, h are x2 - x1, y2 - y1, its score is
 *   class_conf.  A frame is an image iff one of its labels stays; other frames write no record and count nothing.
 *   Per category: the detections that stay, by descending score (the earlier row first on an exact tie), the first 100; IoU in
 *   double on the widened fp32 x y w h; for each of the 10 thresholds iou_thrs (device, double) and 4 area ranges (all, < 32^2,
 *   32^2..96^2, > 96^2 of the fp32 product w*h) the greedy matching of COCOeval.evaluateImg.
 *   rec_key / rec_matched / rec_ignored int64 [F][rec_stride], rec_stride >= min(max_det, 100 * num_classes): the frame's
 *   records category by category in score order.  key = category << 32 | ~(order-preserving bits of the score), so ascending keys
 *   are (category, descending score); bit 4*t + a of matched / ignored is dtMatches != 0 / dtIgnore at threshold t, range a.
 *   Unused slots get key 0x7fffffffffffffff.
 *   counters int32 [96], ADDED to (zero them to start an evaluation): [4k + a] ground truth of category k not ignored in range a,
 *   [64 + k] records of category k, [80] images, [81] images with a detection that stays, [82] truncated frames.
 *   Supported: 1 <= max_det <= 1024, 1 <= G <= 128, 1 <= num_classes <= 16; anything else returns non-zero with the last error
 *   set before any launch.
 *
 * The accumulate entry: perm int64 [n_slots] = the record slots ordered by (key, slot) (a stable sort of rec_key),
 *   rec_thrs double [101] on the device -> precision double [10][101][num_classes][4], COCOeval.accumulate's table at maxDets 100:
 *   -1 where the cell has no non-ignored ground truth.  ws: the ws_bytes query's size (0 = unsupported), contents need not survive.
 *
 * The recall entry: one launch for F frame rows of one stride, one wave per row.
 *   rec_key / rec_matched / rec_ignored int64 [F][rec_stride] exactly as the match entry leaves them (a store whose match calls
 *   used different strides takes one call per run of rows of equal stride).  The rank of a record is its slot minus the first
 *   slot of its category in the row; a record is a true positive at (threshold t, range a) iff bit 4*t + a is set in matched and
 *   clear in ignored.  tp int64 [3][num_classes][40], ADDED to (zero it to start an evaluation) with integer atomics:
 *   tp[m][k][4*t + a] += the true positives of category k with rank < 1, 10, 100 for m = 0, 1, 2.  COCOeval.accumulate's
 *   recall[t][k][a][m] is tp[m][k][4*t + a] / counters[4*k + a] where that count is positive, else -1.  Sums of integers: the
 *   table does not depend on the grid or on the order in which the waves arrive.
 *   Supported: 1 <= rec_stride <= 1024, 1 <= num_classes <= 16, F >= 1; anything else returns non-zero with the last error set
 *   before any launch. */
int rvt_coco_match(const float* det, const int* count, const float* labels, const int* label_count, const long long* t_us, int F,
                   int max_det, int G, int num_classes, int det_xywh, float min_diag, float min_side, const double* iou_thrs,
                   long long* rec_key, long long* rec_matched, long long* rec_ignored, int rec_stride, int* counters, void* stream);
size_t rvt_coco_accumulate_ws_bytes(long long n_slots, int num_classes);
int rvt_coco_accumulate(const long long* perm, const long long* rec_matched, const long long* rec_ignored, long long n_slots,
                        int num_classes, const int* counters, const double* rec_thrs, double* precision, void* ws, size_t ws_bytes,
                        void* stream);
int rvt_coco_recall(const long long* rec_key, const long long* rec_matched, const long long* rec_ignored, int F, int rec_stride,
                    int num_classes, long long* tp, void* stream);

#ifdef __cplusplus
}
#endif
#endif
