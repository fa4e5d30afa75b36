"""Stage-major execution of one backbone stage over a whole event-tensor sequence.

The reference runs time-major: for every time step, all four stages (modules/detection.py:131-148 →
maxvit_rnn.py:93-105).  Only the ConvLSTM is recurrent, and stage s at time t depends on stage s-1 at
the SAME t only, so here each stage processes all T·B frames at once (down-sampling conv + LayerNorm +
window block + grid block as large batched kernels) and then scans its ConvLSTM over t.  The result is
bit-for-bit the same dataflow; it only reorders independent work.  Backward runs stages 4→1, each as a
reverse ConvLSTM scan (BPTT) followed by the batched block / conv backward, so a stage's parameter
gradients are final as soon as that stage is done (used by rvt_amd.dist to overlap the all-reduce).

Layout: activations [T*B][H][W][C] channels-last in the compute dtype; LSTM cell state fp32.
`Hall`/`Call` carry T+1 time slots: slot 0 is the incoming state, slot t+1 the state after step t.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import ops, stage_driver, tuning
from .weights import StageGrads, StageWeights


@dataclass
class StageGeom:
    C: int
    Cin: int
    H_in: int
    W_in: int
    k: int
    stride: int
    pad: int
    ph: int
    pw: int
    dim_head: int
    num_blocks: int
    eps: float

    @property
    def H(self) -> int:
        return (self.H_in + 2 * self.pad - self.k) // self.stride + 1

    @property
    def W(self) -> int:
        return (self.W_in + 2 * self.pad - self.k) // self.stride + 1


class StageSaved:
    """Activations kept for backward (everything else is recomputed from these), and the routes they were produced on."""
    __slots__ = ('inp', 'y0', 'blocks', 'x_last', 'Hall', 'Call', 'gates', 'mask', 'xin_lstm', 'hconv', 'Csave', 'c0', 'routes', 'train', '__weakref__')

    def __init__(self):
        self.blocks: List[Dict[str, Tensor]] = []
        self.routes = None          # stage_driver.RvtStageRoutes of the forward: the ONLY thing the backward chooses its kernels by
        self.train = None           # set by the C-side training driver (rvt_amd/stage_driver.py: train_forward)


def stage_seq_forward(call: stage_driver.StageCall, inp: Tensor, h0: Optional[Tensor], c0: Optional[Tensor],
                      T: int, B: int, save: bool, token_mask: Optional[Tensor] = None,
                      mask_token: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Optional[StageSaved]]:
    """call: the stage's descriptor for this input flavour (weights.ModelWeights.stage_call).  inp: (T*B, H_in, W_in, cin_pad), or the uint8 planes
    (T*B, Cin, h, w) where ops.stem_supported.  Returns Hall (T+1,B,H,W,C), the final cell state (B,H,W,C) fp32, saved."""
    sw, g = call.sw, call.g
    F_ = T * B
    H, W, C = g.H, g.W, g.C
    dt, dev = sw.conv_w.dtype, inp.device
    u8 = inp.dtype == torch.uint8
    r = stage_driver.plan(call, T, B, save, token_mask)
    if save and r.driver_covers and tuning.get('route_stage_driver_train') != 0:
        # the whole training forward of the stage as ONE library call (include/rvt_hip.h: rvt_stage_seq_train_fwd) where covered
        return stage_driver.train_forward(call, r, inp, h0, c0, T, B)
    sv = StageSaved() if save else None
    if save:
        sv.routes = r

    if u8:
        # first stage on the loader's planes (T*B, Cin, h, w): cast + pad + conv + LayerNorm in one launch (csrc/stem.hpp)
        y0, x = ops.stem_fwd(inp, sw.conv_w, sw.ln_w, sw.ln_b, g.H_in, g.W_in, g.eps)
    else:
        y0 = ops.conv_fwd(inp, sw.conv_w, g.k, g.stride, g.pad)                  # maxvit.py:175
        x = ops.layernorm_fwd(y0, sw.ln_w, sw.ln_b, g.eps)                        # maxvit.py:177
    mask_u8 = None
    if token_mask is not None:                                                    # maxvit_rnn.py:174-176
        mask_u8 = token_mask.reshape(F_ * H * W).to(torch.uint8).contiguous()
        ops.token_mask_fwd(x, mask_u8, mask_token.reshape(C).to(torch.float32).contiguous())
    if save:
        sv.inp, sv.y0, sv.mask = inp, y0, mask_u8

    for pair in sw.blocks:
        for bw, window in ((pair[0], True), (pair[1], False)):
            if r.attn_block:
                # maxvit.py:268 in one launch; backward recomputes q / k / v / P from the block input (nothing but `a`,
                # the operand of the proj weight gradient, is kept)
                xmid, a = ops.attn_block_fwd(x, bw['n1_w'], bw['n1_b'], bw['qkv_w'], bw['qkv_b'], bw['proj_w'], bw['proj_b'],
                                             bw['g1'], F_, H, W, C, g.dim_head, g.ph, g.pw, window, g.eps, want_a=save)
                u = qkv = None
            else:
                if r.ln_linear:
                    # norm1 + qkv in one launch (csrc/ln_linear.hpp; C = 128); u is kept for the qkv weight gradient
                    u, qkv = ops.ln_linear_fwd(x, bw['n1_w'], bw['n1_b'], bw['qkv_w'], bw['qkv_b'], g.eps, want_u=save)
                    if bw['n1_w'] is None:
                        u = x
                else:
                    u = x if bw['n1_w'] is None else ops.layernorm_fwd(x, bw['n1_w'], bw['n1_b'], g.eps)
                    qkv = ops.linear_fwd(u, bw['qkv_w'], bw['qkv_b'])                 # maxvit.py:347
                a = ops.attn_fwd(qkv, F_, H, W, C, g.dim_head, g.ph, g.pw, window)    # maxvit.py:349-352
                xmid = ops.linear_scale_res_fwd(a, bw['proj_w'], bw['proj_b'], bw['g1'], x)        # :353, :268
            v2 = None
            if r.mlp_route == 1:
                # the backward recomputes everything from xmid: inference-flavoured forward, nothing else kept (the no-grad
                # forward takes the same kernel, so eval and training outputs are bit-identical)
                xout, hg, hgp = ops.mlp_fwd(xmid, bw['n2_w'], bw['n2_b'], bw['fc1_w'], bw['fc1_b'], bw['fc2_w'], bw['fc2_b'],
                                            bw['g2'], g.eps, want_grad=False)
            elif r.mlp_route == 2:
                # training forward at C = 128: by default only the pre-activation h is kept (hg = h, hgp = None); the backward
                # applies GELU on load in the fc2 weight gradient and GELU' in the epilogue of the fc2 input gradient
                pre = bool(r.mlp_store_pre)
                xout, hg, hgp, v2 = ops.mlp_fwd(xmid, bw['n2_w'], bw['n2_b'], bw['fc1_w'], bw['fc1_b'], bw['fc2_w'], bw['fc2_b'], bw['g2'],
                                                g.eps, want_grad=not pre, want_v2=True, want_pre=pre)      # v2 = LN2(xmid), for the fc1 weight gradient
            else:
                v2 = ops.layernorm_fwd(xmid, bw['n2_w'], bw['n2_b'], g.eps)
                # MLP fc1 + exact GELU; GELU' is saved too so backward never re-evaluates erf (maxvit.py:100-112)
                hg, hgp = ops.linear_gelu_fwd(v2, bw['fc1_w'], bw['fc1_b'], want_grad=save)
                xout = ops.linear_scale_res_fwd(hg, bw['fc2_w'], bw['fc2_b'], bw['g2'], xmid)            # :269
            if save:
                # the LayerNorm outputs are the B operands of the qkv / fc1 weight gradients: kept (1 row of C per token
                # each, 288 GB of HBM) rather than recomputed — a recompute is a read + a write + the re-read
                sv.blocks.append(dict(xin=x, qkv=qkv, a=a, xmid=xmid, hg=hg, hgp=hgp, u=u, v2=v2))
            x = xout

    dws = sw.dws
    # a no-grad forward on the per-step route reads the incoming states where they are (streaming inference, T = 1: the two
    # state copies per stage were 5 % of the step); BPTT and the scan kernel want them in slot 0
    direct0 = (not save) and h0 is not None and r.lstm_route == 0 and h0.dtype == dt and h0.is_contiguous() \
        and c0 is not None and c0.dtype == torch.float32 and c0.is_contiguous()
    lb = stage_driver.LstmBuffers(r, g, dt, dev, T, B, h0, c0, save, direct0)
    Hall, Call, c_last = lb.Hall, lb.Call, lb.c_last
    if r.lstm_route != 0:
        # all T steps in ONE launch: h / c stay on chip, BPTT keeps only a T-typed copy of the cell states (+ the gates where the
        # reverse scan reads them: route 2, weights in the register file; route 3, a wide stage, weights streamed in operand order,
        # gates + cell states saved in dump order)
        xs = x.view(T, B, H, W, C)
        if r.lstm_route == 3:
            ops.lstm_scan3_fwd(xs, Hall, c0, c_last, lb.Csave, sw.scan3_packed(bwd=False), sw.lstm_bn, lb.gates, r.lstm_scan3_rb)
        else:
            ops.lstm_scan_fwd(xs, Hall, c0, c_last, lb.Csave, sw.lstm_wn, sw.lstm_bn, gates_out=lb.gates)
        if save:
            lb.fill_saved(sv, x)
        return Hall, c_last, sv
    # cell states: all T+1 slots are kept for BPTT; a no-grad forward ping-pongs between two
    nc = Call.shape[0]
    # DWS-ConvLSTM (rnn.py:50-54): depth-wise 3x3 on h_{t-1} only, or on cat(x, h_{t-1}) (the x half batched over T)
    x_lstm = x
    hconv = None
    if dws is not None:
        hconv = torch.empty((T if save else 1, B, H, W, C), dtype=dt, device=dev)
        if not dws['only_hidden']:
            x_lstm = ops.dwconv(x, dws['w'][:C], dws['b'][:C], dws['k'])
    xt = x_lstm.view(T, B, H, W, C)
    for t in range(T):                                                            # rnn.py:52-67, one launch per step
        h_prev = h0.view(B, H, W, C) if (direct0 and t == 0) else Hall[t]
        c_prev = c0.view(B, H, W, C) if (direct0 and t == 0) else Call[t % nc]
        h_in = h_prev
        if dws is not None:
            wh = dws['w'] if dws['only_hidden'] else dws['w'][C:]
            bh = dws['b'] if dws['only_hidden'] else dws['b'][C:]
            h_in = ops.dwconv(h_prev, wh, bh, dws['k'], out=hconv[t if save else 0])
        ops.lstm_fwd(xt[t], h_in, c_prev, sw.lstm_w, sw.lstm_b, Hall[t + 1], Call[(t + 1) % nc],
                     lb.gates[t] if save else None)
    if save:
        # the final cell state is handed to the caller (RNNStates keeps it across steps): a buffer of its own, since the
        # T+1-slot array is what BPTT holds on to
        c_last.copy_(Call[T])
        lb.fill_saved(sv, x, x_lstm, hconv)
    return Hall, c_last, sv


def stage_seq_backward(sw: StageWeights, g: StageGeom, sv: StageSaved, dH: Optional[Tensor], dc_last: Optional[Tensor],
                       T: int, B: int, need_input_grad: bool, prev_cot: Optional[Tensor],
                       sg: StageGrads, finalize=None) -> Tuple[Optional[Tensor], Tensor, Tensor]:
    """dH: (T,B,H,W,C) cotangent of Hall[1:] (None = zeros); dc_last: (B,H,W,C) fp32 cotangent of Call[T].
    prev_cot: cotangent already attached to this stage's INPUT frames (T*B,H_in,W_in,Cin) (added to the conv dgrad).
    Parameter gradients are ACCUMULATED into the views of the stage's fp32 bucket, read from its records `sg.stage` / `sg.blocks` under
    the header's slot names (rvt_amd/weights.py: BLOCK_GRADS, STAGE_GRADS, HOST_LOOP_GRADS); `finalize`
    (LayerScale fold + conv unpack, two table launches) runs behind the last weight-gradient GEMM of the stage.
    Returns (d_input or None, dh0, dc0)."""
    F_ = T * B
    H, W, C = g.H, g.W, g.C
    dt, dev = sv.y0.dtype, sv.y0.device
    f32 = torch.float32
    gs = sg.stage
    r = sv.routes                # what the forward was planned with: the tuning record is not consulted again
    if sv.train is not None:
        # BPTT + block / conv backward of the stage as ONE library call (rvt_stage_seq_bwd); the LayerScale fold / conv unpack follow
        out = stage_driver.train_backward(sv, dH, dc_last, T, B, need_input_grad, prev_cot)
        if finalize is not None:
            finalize()
        return out

    # ---- ConvLSTM BPTT ------------------------------------------------------------------------------
    dx = torch.empty((T, B, H, W, C), dtype=dt, device=dev)
    dws = sw.dws
    lstm_wgrad_done = False
    dz = None
    assert (sv.gates is not None) == (r.lstm_route != 1) and (sv.Csave is not None) == (r.lstm_route != 0)
    if r.lstm_route == 3:
        # reverse scan of a wide stage in ONE launch on the saved gates; dz goes to the weight-gradient GEMM below
        dh_rec = torch.empty((B, H, W, C), dtype=dt, device=dev)
        dc_rec = torch.empty((B, H, W, C), dtype=f32, device=dev)
        dz = torch.empty((T, B, H, W, 4 * C), dtype=dt, device=dev)
        ops.lstm_scan3_bwd(sv.gates, sv.Csave, sv.c0, dH, None if dc_last is None else dc_last.to(f32).contiguous(),
                           sw.scan3_packed(bwd=True), dx, dz, dh_rec, dc_rec, r.lstm_scan3_rb)
    elif r.lstm_route != 0:
        # reverse scan in ONE launch: gates recomputed from (x_t, h_{t-1}), dc / dh_rec in registers across t; where built
        # (bf16, C <= 64) the weight gradients are accumulated in the same kernel and dz never exists in HBM
        dh_rec = torch.empty((B, H, W, C), dtype=dt, device=dev)
        dc_rec = torch.empty((B, H, W, C), dtype=f32, device=dev)
        lstm_wgrad_done = bool(r.lstm_scan_wgrad)
        if not lstm_wgrad_done:
            dz = torch.empty((T, B, H, W, 4 * C), dtype=dt, device=dev)
        ops.lstm_scan_bwd(sv.xin_lstm.view(T, B, H, W, C), sv.Hall, sv.Csave, sv.c0, dH,
                          None if dc_last is None else dc_last.to(f32).contiguous(), sw.lstm_wn, sw.lstm_wt, sw.lstm_bn,
                          dx, dz, dh_rec, dc_rec,
                          dw=gs.d_lstm_w if lstm_wgrad_done else None, db=gs.d_lstm_b if lstm_wgrad_done else None, gates=sv.gates)
    else:
        dz = torch.empty((T, B, H, W, 4 * C), dtype=dt, device=dev)
        if dH is None:
            dH = torch.zeros((T, B, H, W, C), dtype=dt, device=dev)
        dc_rec = torch.zeros((B, H, W, C), dtype=f32, device=dev) if dc_last is None else dc_last.to(f32).contiguous().clone()
        dh_rec = None
        dh_buf = [torch.empty((B, H, W, C), dtype=dt, device=dev) for _ in range(2)]
        dhc = torch.empty((T, B, H, W, C), dtype=dt, device=dev) if dws is not None else None   # d(dwconv(h_{t-1}))
        if dws is not None:
            wh = dws['w'] if dws['only_hidden'] else dws['w'][C:]
        for t in range(T - 1, -1, -1):
            ops.lstm_gates_bwd(dH[t], dh_rec, dc_rec, sv.gates[t], sv.Call[t + 1], sv.Call[t], dz[t])
            nxt = dh_buf[t & 1]
            if dws is None:
                ops.lstm_dgrad(dz[t], sw.lstm_wt, dx[t], nxt)
            else:
                ops.lstm_dgrad(dz[t], sw.lstm_wt, dx[t], dhc[t])
                ops.dwconv(dhc[t], wh, None, dws['k'], transpose=True, out=nxt)
            dh_rec = nxt
    if not lstm_wgrad_done:
        h_seg = sv.Hall[:T].reshape(F_, H, W, C) if dws is None else sv.hconv.view(F_, H, W, C)
        ops.lstm_wgrad(dz.view(F_, H, W, 4 * C), sv.xin_lstm, h_seg, gs.d_lstm_w, gs.d_lstm_b)
    dh0, dc0 = dh_rec, dc_rec
    dx = dx.view(F_, H, W, C)
    if dws is not None:
        kk = dws['k']
        cg = dws['w'].shape[0]
        dwd, dbd = gs.d_dws_w.view(cg, kk * kk), gs.d_dws_b
        hprev = sv.Hall[:T].reshape(F_, H, W, C)
        if dws['only_hidden']:
            ops.dwconv_wgrad(hprev, dhc.view(F_, H, W, C), dwd, dbd, kk)
        else:
            ops.dwconv_wgrad(sv.x_last, dx, dwd[:C], dbd[:C], kk)                 # dx here = d(dwconv_x(x))
            ops.dwconv_wgrad(hprev, dhc.view(F_, H, W, C), dwd[C:], dbd[C:], kk)
            dx = ops.dwconv(dx, dws['w'][:C], None, kk, transpose=True)
    del dz

    # ---- attention blocks, reversed ---------------------------------------------------------------------
    dy0_fused = None
    bi_flat = len(sv.blocks)
    for pi in range(len(sw.blocks) - 1, -1, -1):
        for which in (1, 0):
            bw = sw.blocks[pi][which]
            window = which == 0
            bi_flat -= 1
            s = sv.blocks[bi_flat]
            gb = sg.blocks[bi_flat]
            # MLP branch: xout = xmid + g2 * (gelu(hd) W2^T + b2).  The weight-gradient GEMM delivers the raw products
            # S2 = dxout^T g and cs2 = colsum(dxout); LayerScale is folded in by the finalize table launch.
            dn2w, dn2b = gb.d_n2_w, gb.d_n2_b
            assert (s['hg'] is None) == (r.mlp_route == 1) and (s['qkv'] is None) == bool(r.attn_block)
            if r.mlp_route == 1:
                # everything on chip: recompute, both input-gradient products, LayerNorm backward and the fc1 / fc2 weight
                # gradients (accumulated in registers) on chip.  ONE launch where the library supports it (round 4: the
                # weight-gradient kernel hands dh to two waves that form dh W1, LayerNorm backward in the staging role);
                # otherwise two: the weight-gradient half (which needs all 2 x 64 x 256 accumulators), then the input-gradient half
                if r.mlp_bwd_both:
                    dxmid = ops.mlp_bwd_recompute_both(dx, s['xmid'], bw['n2_w'], bw['n2_b'], bw['fc1_w'], bw['fc1_b'], bw['fc2_wt'],
                                                       bw['fc1_wt'], dn2w, dn2b, gb.d_fc1_w, gb.d_fc1_b, gb.d_S2, gb.d_cs2, g.eps)
                else:
                    ops.mlp_bwd_recompute_wgrad(dx, s['xmid'], bw['n2_w'], bw['n2_b'], bw['fc1_w'], bw['fc1_b'],
                                                bw['fc2_wt'], gb.d_fc1_w, gb.d_fc1_b, gb.d_S2, gb.d_cs2, g.eps)
                    dxmid = ops.mlp_bwd_recompute_dgrad(dx, s['xmid'], bw['n2_w'], bw['n2_b'], bw['fc1_w'], bw['fc1_b'],
                                                        bw['fc2_wt'], bw['fc1_wt'], dn2w, dn2b, g.eps)
            else:
                ops.linear_wgrad(dx, s['hg'], gb.d_S2, gelu_in=bool(r.mlp_store_pre), colsum_out=gb.d_cs2)
                fused = bool(r.mlp_bwd_dgrad)
                if fused:       # fc2 dgrad * gp, fc1 dgrad and LayerNorm-2 backward (+ residual) in one kernel
                    dhd, dxmid = ops.mlp_bwd_dgrad(dx, s['hgp'], s['xmid'], bw['n2_w'], bw['fc2_wt'], bw['fc1_wt'], dn2w,
                                                   dn2b, g.eps)
                elif r.mlp_store_pre:
                    dhd = ops.linear_dgrad(dx, bw['fc2_wt'], gelu_pre=s['hg'])
                else:
                    dhd = ops.linear_dgrad(dx, bw['fc2_wt'], mul=s['hgp'])
                v2 = s['v2'] if s['v2'] is not None else ops.layernorm_fwd(s['xmid'], bw['n2_w'], bw['n2_b'], g.eps)
                ops.linear_wgrad(dhd, v2, gb.d_fc1_w, colsum_out=gb.d_fc1_b)
                del v2
                if not fused:
                    if r.dgrad_ln_fc1:     # fc1 input gradient + norm2 backward + residual: one launch
                        dxmid = ops.linear_dgrad_ln(dhd, bw['fc1_w'], s['xmid'], dx, bw['n2_w'], dn2w, dn2b, g.eps)
                    else:
                        dv2 = ops.linear_dgrad(dhd, bw['fc1_wt'])
                        dxmid = ops.layernorm_bwd(s['xmid'], bw['n2_w'], dv2, dx, dn2w, dn2b, g.eps)
                        del dv2
                del dhd
            # attention branch: xmid = xin + g1 * (a Wp^T + bp)
            ops.linear_wgrad(dxmid, s['a'], gb.d_S1, colsum_out=gb.d_cs1)
            if r.attn_block:
                # fused: proj / attention / qkv input gradients and the norm1 backward in one launch (from the block input; a block
                # without norm1 has no d_n1_* either)
                if bi_flat == 0 and r.attn_preln:
                    # the stage's first block: its input is the down-sampling norm's output, and nothing sits between them -
                    # the same launch carries the gradient through that norm (dy0 instead of dx)
                    dy0_fused, dqkv = ops.attn_block_bwd_preln(s['xin'], sv.y0, dxmid, sw.ln_w, bw['qkv_w'], bw['qkv_b'], bw['proj_wt'],
                                                               gs.d_ln_w, gs.d_ln_b, F_, H, W, C, g.dim_head, g.ph, g.pw, window, g.eps)
                    dx, u = None, None
                else:
                    dy0_fused = None
                    dx, dqkv, u = ops.attn_block_bwd(s['xin'], dxmid, bw['n1_w'], bw['n1_b'], bw['qkv_w'], bw['qkv_b'], bw['proj_wt'],
                                                     gb.d_n1_w, gb.d_n1_b, F_, H, W, C, g.dim_head, g.ph, g.pw, window, g.eps)
                u = s['xin'] if u is None else u
                ops.linear_wgrad(dqkv, u, gb.d_qkv_w, colsum_out=gb.d_qkv_b)
                del dqkv, dxmid, u
                continue
            da = ops.linear_dgrad(dxmid, bw['proj_wt'])
            dqkv = ops.attn_bwd(s['qkv'], da, F_, H, W, C, g.dim_head, g.ph, g.pw, window)
            del da
            ops.linear_wgrad(dqkv, s['u'], gb.d_qkv_w, colsum_out=gb.d_qkv_b)
            if bi_flat == 0 and r.attn_preln:
                # the stage's first block: qkv input gradient + residual cotangent carried through the down-sampling norm (one launch)
                dy0_fused = ops.linear_dgrad_preln(dqkv, bw['qkv_w'], sv.y0, dxmid, sw.ln_w, gs.d_ln_w, gs.d_ln_b, g.eps)
                dx = None
            elif bw['n1_w'] is None:
                dx = ops.linear_dgrad(dqkv, bw['qkv_wt'], add=dxmid)
            elif r.dgrad_ln_qkv:           # qkv input gradient + norm1 backward + residual: one launch
                dx = ops.linear_dgrad_ln(dqkv, bw['qkv_w'], s['xin'], dxmid, bw['n1_w'], gb.d_n1_w, gb.d_n1_b, g.eps)
            else:
                du = ops.linear_dgrad(dqkv, bw['qkv_wt'])
                dx = ops.layernorm_bwd(s['xin'], bw['n1_w'], du, dxmid, gb.d_n1_w, gb.d_n1_b, g.eps)
                del du
            del dqkv, dxmid

    # ---- token mask, down-sampling LayerNorm + conv ---------------------------------------------------------
    if sv.mask is not None:
        ops.token_mask_bwd(dx, sv.mask, gs.d_mask_token.view(C))            # also zeroes dx on masked tokens
    if dy0_fused is not None:
        dy0 = dy0_fused                                                           # (rvt_attn_block_bwd_preln of the first block)
    else:
        dy0 = ops.layernorm_bwd(sv.y0, sw.ln_w, dx, None, gs.d_ln_w, gs.d_ln_b, g.eps)
    if sv.inp.dtype == torch.uint8:
        ops.stem_wgrad(sv.inp, dy0, gs.d_raw_conv, g.H_in, g.W_in)
    else:
        ops.conv_wgrad(sv.inp, dy0, gs.d_raw_conv, g.k, g.stride, g.pad)
    if finalize is not None:
        finalize()               # in stream order behind every weight-gradient GEMM of this stage
    d_in = None
    if need_input_grad:
        if r.conv_dgrad4:
            d_in = ops.conv_dgrad4(dy0, sw.conv_wd4, prev_cot, g.H_in, g.W_in, g.Cin)      # one launch (2 x 2 pixel blocks)
        else:
            d_in = ops.conv_dgrad(dy0, sw.conv_wd, prev_cot, g.H_in, g.W_in, g.Cin, g.k, g.stride, g.pad)
    return d_in, dh0, dc0        # every parameter gradient of this stage is final from here on (DDP hook, optimizer)
