"""Algorithmic FLOP / HBM-byte model of EVERY C-ABI entry point (include/rvt_hip.h), for bench.py's `roofline` objects.

MEASUREMENT INFRASTRUCTURE (not part of the product path).  Round 3's bench could only price GEMM-family launches, so its
`roofline` could never name the worst kernels.  `model(name, args)` returns, from the launch's own
arguments (read by the parameter names of include/rvt_hip.h, never by position):

  flops  ALGORITHMIC MFMA-side work of the operator, 2*MAC: the products the reference's forward / autograd
         performs for the same result - e.g. 16 M C^2 for each of {MLP forward, its input gradients, its weight gradients}.
         Products a recompute-style backward re-does (fc1 / GELU recomputed from xmid, q / k / v / P recomputed from the block
         input, ConvLSTM gates recomputed in the reverse scan) are NOT counted here: `executed(name, args)` returns the
         recompute-inclusive figure separately (round 5; the round-4 line priced the recompute as algorithmic work and
         printed 0.20 where 0.16 was right).  Element-wise work (LayerNorm, softmax, GELU, gates) is not counted.
  bytes  algorithmic HBM bytes: every operand and result tensor crosses HBM exactly once (weights once per launch);
         intermediates that the operator's definition keeps on chip are not counted.
  Roof: arithmetic intensity flops/bytes against the ridge peak_flops / 8 TB/s decides which roof bounds the launch.

DESIGN.md §4 lists the per-unit figures these formulas implement.
"""
from __future__ import annotations

from typing import Optional, Tuple

from rvt_amd._header import ENUMS, LaunchArgs

HBM_PEAK_GBS = 8000.0                             # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6.3 TB/s achievable
PEAK_TFLOPS = {'bf16': 2500.0, 'f32': 157.3}      # dense MFMA peaks at 2.4 GHz
_OPTIM_CHUNK = ENUMS['RVT_OPTIM_CHUNK_ELEMS']


def _elt(dtype_code: int) -> int:
    return 4 if dtype_code == 0 else 2


def _conv_out(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _price(name: str, a) -> Optional[Tuple[float, float, float]]:
    """(algorithmic flops, bytes, flops a recompute adds on top) of one launch; `a` = the launch's arguments by the header's
    parameter names (rvt_amd/_header.py: LaunchArgs).  None for an entry point with no model."""
    if name == 'rvt_stem_fwd':
        e, F, Cin = _elt(a.dtype), a.F, a.Cin
        Ho, Wo = _conv_out(a.H, a.W, 7, 4, 3)
        return 2.0 * F * Ho * Wo * 64 * Cin * 49, F * Cin * a.h * a.wd + 2.0 * F * Ho * Wo * 64 * e + 64 * 49 * Cin * e, 0.0
    if name == 'rvt_stem_wgrad':
        e, F, Cin = _elt(a.dtype), a.F, a.Cin
        Ho, Wo = _conv_out(a.H, a.W, 7, 4, 3)
        return 2.0 * F * Ho * Wo * 64 * Cin * 49, F * Cin * a.h * a.wd + 1.0 * F * Ho * Wo * 64 * e + 64 * 49 * Cin * 4, 0.0
    if name == 'rvt_prepack_input':                      # src_kind 0 = float32 planes, else one byte per element
        return 0.0, a.F * a.Cin * a.h * a.w * (1 if a.src_kind else 4) + 1.0 * a.F * a.H * a.W * a.Cp * _elt(a.dtype), 0.0
    if name in ('rvt_conv_fwd', 'rvt_conv_wgrad', 'rvt_conv_dgrad'):
        e, F, H, W, Cin, Cout, k = _elt(a.dtype), a.F, a.H, a.W, a.Cin, a.Cout, a.k
        Ho, Wo = _conv_out(H, W, k, a.stride, a.pad)
        fl = 2.0 * F * Ho * Wo * Cout * Cin * k * k
        by = 1.0 * F * H * W * Cin * e + 1.0 * F * Ho * Wo * Cout * e + Cout * Cin * k * k * (4 if name.endswith('wgrad') else e)
        if name == 'rvt_conv_dgrad' and a.has('add'):
            by += 1.0 * F * H * W * Cin * e
        return fl, by, 0.0
    if name == 'rvt_conv_dgrad4':
        e, F, H, W, Cin, Cout = _elt(a.dtype), a.F, a.H, a.W, a.Cin, a.Cout
        by = 1.0 * F * H * W * Cin * e * (2 if a.has('add') else 1) + 1.0 * F * (H // 2) * (W // 2) * Cout * e + 9 * Cout * Cin * e
        return 2.0 * F * (H // 2) * (W // 2) * Cout * Cin * 9, by, 0.0
    if name == 'rvt_layernorm_fwd':
        return 0.0, 2.0 * a.rows * a.C * _elt(a.dtype), 0.0
    if name == 'rvt_layernorm_bwd':
        return 0.0, (3.0 + (1 if a.has('dres') else 0)) * a.rows * a.C * _elt(a.dtype), 0.0
    if name == 'rvt_linear_fwd':
        e, M, N, K = _elt(a.dtype), a.M, a.N, a.K
        return 2.0 * M * N * K, (1.0 * M * (N + K) + N * K) * e, 0.0
    if name == 'rvt_ln_linear_fwd':                      # u = LN(x), y = u w^T + bias
        e, M, C, N = _elt(a.dtype), a.M, a.C, a.N
        return 2.0 * M * N * C, (1.0 * M * (C * (2 if a.has('u') and a.has('ln_w') else 1) + N) + N * C) * e, 0.0
    if name == 'rvt_linear_gelu_fwd':
        e, M, N, K = _elt(a.dtype), a.M, a.N, a.K
        return 2.0 * M * N * K, (1.0 * M * (N * (2 if a.has('gp') else 1) + K) + N * K) * e, 0.0
    if name == 'rvt_linear_scale_res_fwd':
        e, M, N, K = _elt(a.dtype), a.M, a.N, a.K
        return 2.0 * M * N * K, (1.0 * M * (2 * N + K) + N * K) * e, 0.0
    if name == 'rvt_linear_dgrad':                       # dx[M][K] = dy[M][N] wt[K][N]^T (* gelu' | + add | * mul)
        e, M, N, K = _elt(a.dtype), a.M, a.N, a.K
        side = 1 if (a.has('gelu_pre') or a.has('add') or a.has('mul')) else 0
        return 2.0 * M * N * K, (1.0 * M * (N + K * (1 + side)) + N * K) * e, 0.0
    if name == 'rvt_linear_dgrad_preln':                 # dy0 = LN'(dy w + add; y0): same rows as the form below with add
        e, M, C, K = _elt(a.dtype), a.M, a.C, a.K
        return 2.0 * M * C * K, (1.0 * M * (K + 3 * C) + K * C) * e, 0.0
    if name == 'rvt_linear_dgrad_ln':                    # dx = add + LN'(dy w; x)
        e, M, C, K = _elt(a.dtype), a.M, a.C, a.K
        return 2.0 * M * C * K, (1.0 * M * (K + C * (2 + (1 if a.has('add') else 0))) + K * C) * e, 0.0
    if name == 'rvt_linear_wgrad':
        e, M, N, K = _elt(a.dtype), a.M, a.N, a.K
        return 2.0 * M * N * K, 1.0 * M * (N + K) * e + 4.0 * N * K, 0.0
    if name == 'rvt_mlp_fwd':                            # LN2 -> fc1 -> GELU -> fc2 -> gamma, + residual
        e, M, C = _elt(a.dtype), a.M, a.C
        rows = 2 + ((8 if a.has('gp_out') else 4) if a.has('g_out') else 0) + (1 if a.has('v2_out') else 0)        # (g_out alone = the pre-activation only)
        return 16.0 * M * C * C, (1.0 * rows * M * C + 8 * C * C) * e, 0.0
    if name == 'rvt_mlp_bwd_dgrad':                      # fc2 dgrad * gp -> dh (stored) -> fc1 dgrad -> LN2' + residual
        e, M, C = _elt(a.dtype), a.M, a.C
        return 16.0 * M * C * C, (11.0 * M * C + 8 * C * C) * e, 0.0
    if name == 'rvt_mlp_bwd_recompute_dgrad':            # both input gradients (16); recompute of fc1 (8)
        e, M, C = _elt(a.dtype), a.M, a.C
        return 16.0 * M * C * C, (3.0 * M * C + 12 * C * C) * e, 8.0 * M * C * C
    if name == 'rvt_mlp_bwd_recompute_wgrad':            # both weight gradients (16); recompute of fc1 (8) + fc2 dgrad for dh (8)
        e, M, C = _elt(a.dtype), a.M, a.C
        return 16.0 * M * C * C, 2.0 * M * C * e + 8.0 * C * C * (e + 4), 16.0 * M * C * C
    if name == 'rvt_mlp_bwd_recompute_both':             # input + weight gradients (32); recompute of fc1 (8)
        e, M, C = _elt(a.dtype), a.M, a.C
        return 32.0 * M * C * C, 3.0 * M * C * e + 8.0 * C * C * (e + 4), 8.0 * M * C * C
    if name in ('rvt_attn_fwd', 'rvt_attn_bwd', 'rvt_attn_block_fwd', 'rvt_attn_block_bwd', 'rvt_attn_block_bwd_preln'):
        e, F, H, W, C, L = _elt(a.dtype), a.F, a.H, a.W, a.C, a.ph * a.pw
        M = F * H * W                                    # (the recompute terms below keep the parent formulas' own spelling, F * H * W * ph * pw:
                                                         #  the same product in another order can differ in the last bit)
        if name == 'rvt_attn_fwd':
            return 4.0 * M * L * C, 4.0 * M * C * e, 0.0
        if name == 'rvt_attn_bwd':                       # dV, dP, dQ, dK (8 L C); recompute of S (2)
            return 8.0 * M * L * C, 7.0 * M * C * e, 2.0 * F * H * W * a.ph * a.pw * C
        if name == 'rvt_attn_block_fwd':                 # LN1 -> qkv (6C^2) -> attention (4LC) -> proj (2C^2) -> gamma + residual
            return M * (8.0 * C * C + 4.0 * L * C), ((2.0 + (1 if a.has('a_out') else 0)) * M * C + 4 * C * C) * e, 0.0
        recompute = F * H * W * (6.0 * C * C + 2.0 * a.ph * a.pw * C)             # of qkv (6C^2) + S (2LC)
        if name == 'rvt_attn_block_bwd':                 # dproj (2C^2), core (8LC), du (6C^2)
            return M * (8.0 * C * C + 8.0 * L * C), ((6.0 + (1 if a.has('u_out') else 0)) * M * C + 7 * C * C) * e, recompute
        return M * (8.0 * C * C + 8.0 * L * C), (7.0 * M * C + 7 * C * C) * e, recompute      # _preln: the same products; rows: x, y0, dxmid in, dy0 + dqkv (3) out
    if name == 'rvt_lstm_fwd':
        e, M, C = _elt(a.dtype), a.M, a.C
        return 16.0 * M * C * C, 1.0 * M * C * (3 * e + 8 + (4 * e if a.has('gates') else 0)) + 8.0 * C * C * e, 0.0
    if name == 'rvt_lstm_gates_bwd':
        e, M, C = _elt(a.dtype), a.M, a.C
        return 0.0, 1.0 * M * C * ((1 + (1 if a.has('dh_rec') else 0) + 8) * e + 16), 0.0
    if name == 'rvt_lstm_dgrad':
        e, M, C = _elt(a.dtype), a.M, a.C
        return 16.0 * M * C * C, (6.0 * M * C + 8 * C * C) * e, 0.0
    if name == 'rvt_lstm_wgrad':
        e, M, C = _elt(a.dtype), a.M, a.C
        return 16.0 * M * C * C, 6.0 * M * C * e + 32.0 * C * C, 0.0
    if name == 'rvt_lstm_scan_fwd':                      # per token-step: x in, h out (+ c copy, + gates) — h / c stay on chip
        e, M, C, T = _elt(a.dtype), a.M, a.C, a.T_steps
        rows = 2 + (1 if a.has('Csave') else 0) + (4 if a.has('gates_out') else 0)
        return 16.0 * M * C * C * T, 1.0 * rows * M * C * T * e + 8.0 * M * C + 8 * C * C * e, 0.0
    if name == 'rvt_lstm_scan_bwd':
        e, M, C, T = _elt(a.dtype), a.M, a.C, a.T_steps
        saved_gates = a.has('gates')
        fl = 16.0 + (16.0 if a.has('dw') else 0.0)                           # dgrad (+ in-kernel weight gradient)
        rows = (2 + 4 if saved_gates else 4) + 1 + (4 if a.has('dz_all') else 0)        # (c, dH, gates | x, h, c, dH) in, dx out (+ dz out)
        return (fl * M * C * C * T, 1.0 * rows * M * C * T * e + 16.0 * M * C + 16 * C * C * e,
                0.0 if saved_gates else 16.0 * M * C * C * T)                           # gate recompute (16) unless the gates were saved
    if name == 'rvt_lstm_scan3_fwd':                     # wide stages: x in, h out (+ bf16 c copy + 4 activated gates when saving); weights once
        e, M, C, T = _elt(a.dtype), a.M, a.C, a.T_steps
        rows = 2 + (5 if a.has('gsave') else 0)
        return 16.0 * M * C * C * T, 1.0 * rows * M * C * T * e + 8.0 * M * C + 8 * C * C * e, 0.0
    if name == 'rvt_lstm_scan3_bwd':                     # gates (4) + c + dH in, dz (4) + dx out; W^T once
        e, M, C, T = _elt(a.dtype), a.M, a.C, a.T_steps
        rows = 4 + 1 + (1 if a.has('dH') else 0) + 4 + 1
        return 16.0 * M * C * C * T, 1.0 * rows * M * C * T * e + 16.0 * M * C + 8 * C * C * e, 0.0
    if name == 'rvt_lstm_scan3_pack':
        return 0.0, 8.0 * a.C * a.C * 2 * (1 + (1 if a.has('wp_fwd') else 0) + (1 if a.has('wtp_bwd') else 0)), 0.0
    if name in ('rvt_dwconv_fwd', 'rvt_dwconv_wgrad'):
        return 0.0, 2.0 * a.N * a.H * a.W * a.C * _elt(a.dtype), 0.0
    if name in ('rvt_token_mask_fwd', 'rvt_token_mask_bwd'):
        return 0.0, 1.0 * a.M * a.C * _elt(a.dtype), 0.0
    # ---- detection tail (rows f2 / f3): BatchNorm + SiLU row kernels around the PAFPN / head convolutions, decode, SimOTA + losses
    if name == 'rvt_bn_stats':                                   # one read of the conv output
        return 0.0, 1.0 * a.rows * a.C * _elt(a.dtype), 0.0
    if name == 'rvt_bn_act_fwd':                                 # read + write
        return 0.0, 2.0 * a.rows * a.C * _elt(a.dtype), 0.0
    if name == 'rvt_bn_act_bwd_stats':                           # dy and x in
        return 0.0, 2.0 * a.rows * a.C * _elt(a.dtype), 0.0
    if name == 'rvt_bn_act_bwd_apply':                           # dy and x in, dx out
        return 0.0, 3.0 * a.rows * a.C * _elt(a.dtype), 0.0
    if name == 'rvt_bn_finalize':
        return 0.0, 48.0 * a.C, 0.0                              # two fp64 sums in; running statistics, four fp32 vectors out
    if name in ('rvt_yolox_decode', 'rvt_yolox_decode_bwd'):     # the level's two prediction maps <-> [B][A][5+nc] fp32 rows
        outs = (1 if a.has('pred_train') else 0) + (1 if a.has('pred_infer') else 0) if name == 'rvt_yolox_decode' else 2
        return 0.0, 1.0 * a.B * a.H * a.W * ((a.ld_ro + a.ld_cls) * _elt(a.dtype) + outs * (5 + a.num_classes) * 4), 0.0
    if name == 'rvt_simota_loss':                                # pred in (cost, select/resolve, loss passes), cost + IoU matrices out and back
        B, G, A, nc = a.B, a.G, a.A, a.num_classes
        return 0.0, 3.0 * B * A * (5 + nc) * 4 + (B * A * (5 + nc) * 4 if a.has('g_pred') else 0) + 4.0 * B * G * A * 4 + 6.0 * B * A * 4, 0.0
    # post-processing: the executed figure is vector (not MFMA) work, data dependent: the all-pairs bound of the greedy NMS, 12 flops
    # per IoU test (4 min/max, 3 sub, 2 max, mul, add, div)
    if name == 'rvt_yolox_postprocess':                          # pred in, det / count / anchor_idx out, the workspace written and read back
        B, A, nc, max_det = a.B, a.A, a.num_classes, a.max_det
        by = 1.0 * B * A * (5 + nc) * 4 + B * max_det * 7 * 4 + B * 4 + (B * max_det * 4 if a.has('anchor_idx') else 0) + 2.0 * 52 * B * A
        return 0.0, by, 12.0 * B * A * (A - 1) / 2
    if name == 'rvt_yolox_detect':                               # the levels' maps read once (A rows per image over all levels), det / count /
        B, A, nc, max_det = a.B, a.A, a.num_classes, a.max_det   # anchor_idx out, the workspace written and read back
        by = (1.0 * B * A * (a.ld_ro + a.ld_cls) * _elt(a.dtype) + B * max_det * 7 * 4 + B * 4 + (B * max_det * 4 if a.has('anchor_idx') else 0)
              + 2.0 * 52 * B * A)
        return 0.0, by, 12.0 * B * A * (A - 1) / 2 + 3.0 * B * A * (1 + nc)      # + one sigmoid (exp, add, divide: 3) per class and objectness logit
    if name == 'rvt_augment_planes':                             # uint8 planes in and out; the per-sample windows live in the device table,
        return 0.0, 2.0 * a.F * a.C * a.H * a.W + 32.0 * a.B, 0.0          # so this is the bound of a flip: every byte read once, written once
    if name == 'rvt_augment_labels':                             # rows + count in, rows + count (+ yolox) out
        F, B, G = a.F, a.B, a.G
        return 0.0, 2.0 * F * (G * 7 * 4 + 4) + (F * G * 5 * 4 if a.has('yolox_out') else 0) + 48.0 * B, 0.0
    if name == 'rvt_coco_match':                                 # det + count, label rows + count, timestamps in; the frame's record slots out
        F, max_det, G = a.F, a.max_det, a.G
        return 0.0, 1.0 * F * (max_det * 7 * 4 + 4 + G * 7 * 4 + 4 + 8) + 24.0 * F * a.rec_stride + 80.0, 0.0
    if name == 'rvt_coco_accumulate':                            # permutation + the two mask planes read twice (count, emit); table out
        return 0.0, 2.0 * 24 * a.n_slots + 10 * 101 * a.num_classes * 4 * 8.0, 0.0
    if name == 'rvt_coco_recall':                                # the three record planes in (a wave's second look at its key row is on chip); table added to
        return 0.0, 24.0 * a.F * a.rec_stride + 2.0 * 3 * a.num_classes * 40 * 8, 0.0
    # sparse frame cache: no nnz among the arguments, so a launch is priced at what its arrays admit (pack: every byte non-zero up to
    # `capacity`; unpack: the whole values array read).  frames_pack_bytes / frames_unpack_bytes take the measured nnz.
    if name == 'rvt_frames_pack':
        return 0.0, frames_pack_bytes(a.F, a.E, min(a.capacity, a.F * a.E)), 0.0
    if name == 'rvt_frames_unpack':
        return 0.0, frames_unpack_bytes(a.Fout, a.E, a.values_len), 0.0
    if name == 'rvt_frames_unpack_augment':                      # the same bound, plus the table; the windows live in the device table
        return 0.0, frames_unpack_augment_bytes(a.Fout, a.E, a.values_len, a.B), 0.0
    if name == 'rvt_frames_gather':                              # the counts live in the device table: every frame full up to `capacity`
        return 0.0, frames_gather_bytes(a.n, a.E, min(a.capacity, a.n * a.E)), 0.0
    # format version 2: neither nnz nor ngroups among the arguments, so the same bounds (every byte and every group live up to the
    # two capacities; unpack: both arrays read whole).  frames_*2_bytes take the measured counts.
    if name == 'rvt_frames_pack2':
        return 0.0, frames_pack2_bytes(a.F, a.E, min(a.mask_capacity, a.F * ((a.E + 63) // 64)), min(a.capacity, a.F * a.E)), 0.0
    if name == 'rvt_frames_unpack2':
        return 0.0, frames_unpack2_bytes(a.Fout, a.E, a.masks_len, a.values_len), 0.0
    if name == 'rvt_frames_gather2':
        return 0.0, frames_gather2_bytes(a.n, a.E, min(a.mask_capacity, a.n * ((a.E + 63) // 64)), min(a.capacity, a.n * a.E)), 0.0
    if name == 'rvt_render_preview':                             # the planes of every rendered frame read once for all panels, the images written once
        return 0.0, render_preview_bytes(a.Fout, a.C, a.H, a.W, a.P, a.scale), 0.0
    # the optimizer's chunk table: no element count among the arguments, so a launch is priced at what its table admits (every chunk
    # full).  grad_stats_bytes / optim_step_bytes take the real element count.
    if name == 'rvt_grad_stats':
        return 0.0, grad_stats_bytes(a.n_chunks * _OPTIM_CHUNK, a.n_chunks, a.n_tensors), 0.0
    if name == 'rvt_optim_step_guarded':                         # the step it is when the verdict is clean; a skipped one reads 8 bytes per workgroup
        return 0.0, optim_step_bytes(a.n_chunks * _OPTIM_CHUNK, a.n_chunks), 0.0
    return None


def model(name: str, args) -> Optional[Tuple[float, float]]:
    """(flops, bytes) of one launch from its positional arguments as `_lib.call` sees them, or None for an entry point with no model
    (host-side tables, size queries)."""
    m = _price(name, LaunchArgs(name, args))
    return None if m is None else m[:2]


def augment_planes_bytes(F: int, C: int, H: int, W: int, windows) -> float:
    """HBM bytes of one rvt_augment_planes launch when the table is known: windows[b] = (mode, zh, zw) of sample b = f % B.
    Every output byte is written once; a zoom-in reads its zh x zw source window, a zoom-out the zh source rows it keeps."""
    total = 0.0
    for f in range(F):
        mode, zh, zw = windows[f % len(windows)]
        read = {1: zh * zw, 2: zh * W}.get(mode, H * W)
        total += C * (H * W + read)
    return total


def _frames_meta_bytes(E: int) -> int:
    """masks + seg_offset + one value_base entry of one frame of E bytes (format version 1, include/rvt_hip.h)."""
    Gf = (E + 63) // 64
    Sf = (Gf + 63) // 64
    return 8 * Gf + 4 * (Sf + 1) + 8


def frames_pack_bytes(F: int, E: int, nnz: int) -> float:
    """HBM bytes of one rvt_frames_pack when nnz is known: the dense frames read twice (masks, then compaction) and the packed set
    (8 Gf F + 4 (Sf + 1) F + 8 (F + 1) + nnz) written once.  The workspace (4 bytes per segment, written and read) is not counted."""
    return 2.0 * F * E + F * _frames_meta_bytes(E) + 8 + nnz


def frames_unpack_bytes(Fout: int, E: int, nnz: int) -> float:
    """HBM bytes of one rvt_frames_unpack that fetches Fout frames holding nnz non-zero bytes between them: their masks, seg_offset
    rows, value_base entries and index entries read, their values read, the dense frames written."""
    return 1.0 * Fout * E + Fout * (_frames_meta_bytes(E) + 8) + nnz


def frames_unpack_augment_bytes(Fout: int, E: int, nnz: int, B: int) -> float:
    """HBM bytes of one rvt_frames_unpack_augment: what frames_unpack_bytes counts (the dense frames written once, the fetched
    frames' metadata and their nnz value bytes read) plus the int32 [B][8] table.  No dense intermediate is written or read."""
    return frames_unpack_bytes(Fout, E, nnz) + 32.0 * B


def frames_gather_bytes(n: int, E: int, nnz: int) -> float:
    """Bytes of one rvt_frames_gather that fetches n frames holding nnz non-zero bytes between them: their packed bytes (masks,
    seg_offset rows, value_base, values: 8 Gf n + 4 (Sf + 1) n + 8 (n + 1) + nnz) read once and written once, plus the int64 [n][4]
    table.  The reads cross the host link when the stores are pinned host memory; the writes are HBM's."""
    return 2.0 * (n * _frames_meta_bytes(E) + 8 + nnz) + 32.0 * n


def _frames2_meta_bytes(E: int) -> int:
    """group_mask, seg_offset and grp_offset rows plus one value_base and one mask_base entry of one frame of E bytes (format
    version 2, include/rvt_hip.h): 16 Sf + 8 + 16."""
    Sf = ((E + 63) // 64 + 63) // 64
    return 8 * Sf + 2 * 4 * (Sf + 1) + 16


def frames_pack2_bytes(F: int, E: int, ngroups: int, nnz: int) -> float:
    """HBM bytes of one rvt_frames_pack2 when the counts are known: the dense frames read twice (group masks, then compaction: the
    masks are recomputed, not kept) and the packed set (16 Sf F + 8 F + 16 (F + 1) + 8 ngroups + nnz) written once.  The workspace
    (8 bytes per segment, written and read) is not counted."""
    return 2.0 * F * E + F * _frames2_meta_bytes(E) + 16 + 8 * ngroups + nnz


def frames_unpack2_bytes(Fout: int, E: int, ngroups: int, nnz: int) -> float:
    """HBM bytes of one rvt_frames_unpack2 that fetches Fout frames holding ngroups non-empty groups and nnz non-zero bytes between
    them: their rows, base entries and index entries read, their masks and values read, the dense frames written."""
    return 1.0 * Fout * E + Fout * (_frames2_meta_bytes(E) + 8) + 8 * ngroups + nnz


def frames_gather2_bytes(n: int, E: int, ngroups: int, nnz: int) -> float:
    """Bytes of one rvt_frames_gather2 that fetches n frames holding ngroups non-empty groups and nnz non-zero bytes between them:
    their packed bytes read once and written once, plus the int64 [n][8] table.  The reads cross the host link when the stores are
    pinned host memory; the writes are HBM's."""
    return 2.0 * (n * _frames2_meta_bytes(E) + 16 + 8 * ngroups + nnz) + 64.0 * n


def render_preview_bytes(Fout: int, C: int, H: int, W: int, P: int, scale: int) -> float:
    """HBM bytes of one rvt_render_preview: the C byte planes of each of the Fout rendered frames read once, the P panels of
    (H scale) x (W scale) RGB pixels written once.  (Box rows, counts, the index and the three small tables: not counted.)"""
    return 1.0 * Fout * C * H * W + 3.0 * Fout * P * H * scale * W * scale


def grad_stats_bytes(n_elems: int, n_chunks: int, n_tensors: int) -> float:
    """HBM bytes of one rvt_grad_stats over n_elems fp32 elements in n_chunks chunks of n_tensors tensors: gradient and parameter read
    once (8 bytes per element), the chunk table read (40 per row), one 32-byte partial row per chunk written and read back, one
    32-byte row per tensor, the 64-byte head and the verdict written.  (tensor_first, the scalars and the step count: not counted.)"""
    return 8.0 * n_elems + 40.0 * n_chunks + 2 * 32.0 * n_chunks + 32.0 * n_tensors + 64 + 8


def optim_step_bytes(n_elems: int, n_chunks: int) -> float:
    """HBM bytes of one rvt_optim_step / rvt_optim_step_guarded that steps: 16 bytes read and 12 written per element (csrc/optim.hpp)
    plus the chunk table."""
    return 28.0 * n_elems + 40.0 * n_chunks


def executed(name: str, args) -> Optional[float]:
    """MFMA-side FLOPs the launch actually EXECUTES: model()'s algorithmic figure plus the products a recompute-style backward
    re-does by design.  Equal to the algorithmic figure for every other entry point."""
    m = _price(name, LaunchArgs(name, args))
    return None if m is None else m[0] + m[2]


def roofline_entry(name: str, flops: float, bytes_: float, ms: float, launches: int, dtype: str, mfma_peak_tflops: float = None,
                   executed_flops: float = None):
    """One roofline record for `launches` launches that took `ms` in total.  `flops` = ALGORITHMIC (what `frac` is computed from);
    `executed_flops` (optional) = recompute-inclusive, reported beside it."""
    peak = mfma_peak_tflops or PEAK_TFLOPS[dtype]
    tfl = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    gbs = bytes_ / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    ai = flops / bytes_ if bytes_ > 0 else float('inf')
    ridge = peak * 1e12 / (HBM_PEAK_GBS * 1e9)
    bound = 'hbm' if ai < ridge else 'mfma'
    rec = {'kernel': name, 'bound': bound, 'launches': launches, 'ms': round(ms, 4), 'avg_launch_ms': round(ms / max(launches, 1), 4),
           'algorithmic_gflop': round(flops / 1e9, 2), 'algorithmic_gbyte': round(bytes_ / 1e9, 3),
           'arithmetic_intensity_flop_per_byte': round(ai, 1) if ai != float('inf') else None,
           'hbm_gbs': round(gbs, 1), 'hbm_frac': round(gbs / HBM_PEAK_GBS, 4),
           'mfma_tflops': round(tfl, 2), 'mfma_frac': round(tfl / peak, 4)}
    if executed_flops is not None and executed_flops != flops:
        rec['executed_gflop'] = round(executed_flops / 1e9, 2)
        rec['executed_mfma_tflops'] = round(executed_flops / (ms * 1e-3) / 1e12, 2) if ms > 0 else 0.0
    if bound == 'hbm':
        rec.update(achieved=round(gbs, 1), peak=HBM_PEAK_GBS, unit='GB/s', frac=round(gbs / HBM_PEAK_GBS, 4))
    else:
        rec.update(achieved=round(tfl, 2), peak=peak, unit='TFLOP/s', frac=round(tfl / peak, 4))
    return rec
