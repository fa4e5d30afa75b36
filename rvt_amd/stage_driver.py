"""Binding of the C-side stage drivers (include/rvt_hip.h) and of the route planner they share with the host loop.

  * plan(): the routes of one stage, decided ONCE per forward by the library (rvt_stage_routes) and kept with the saved activations
    (StageSaved.routes), so that the backward runs what the forward prepared for;
  * stage_seq_fwd(): the no-grad forward of one stage over a whole sequence as ONE library call (validation / streaming inference,
    reference modules/detection.py:231-255);
  * train_forward() / train_backward(): the training forward and the BPTT backward as one call each, where routes.driver_covers.

rvt_amd/stage.py is the operator-by-operator host loop for everything else (token masks, DWS-ConvLSTM, the saving fused-MLP
flavour).  Python only allocates: outputs, saved activations and a grow-only workspace per stream."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib as L, tuning
from ._header import STRUCTS, fields

RvtBlockWeights, RvtStageDesc, RvtStageRoutes, RvtBlockSaved, RvtBlockTrain, RvtStageTrain = (
    STRUCTS[n] for n in ('RvtBlockWeights', 'RvtStageDesc', 'RvtStageRoutes', 'RvtBlockSaved', 'RvtBlockTrain', 'RvtStageTrain'))


class StageCall:
    """Descriptor of one stage for one input flavour; keeps the host-side block array (and through `sw` the device tensors) alive.
    Built and kept by weights.ModelWeights.stage_call; `train`: the stage's TrainTables where the weight set has gradient buckets."""

    def __init__(self, sw, g, dtype: torch.dtype, inp_u8: bool, h_raw: int, w_raw: int, train: Optional['TrainTables'] = None):
        p = L.ptr
        nb = 2 * g.num_blocks
        self.blocks = (RvtBlockWeights * max(nb, 1))()
        i = 0
        for pair in sw.blocks:
            for bw in pair:
                b = self.blocks[i]
                for k in fields(RvtBlockWeights):
                    setattr(b, k, p(bw[k]))
                i += 1
        d = RvtStageDesc()
        d.struct_bytes = ctypes.sizeof(RvtStageDesc)
        d.dtype, d.C, d.Cin, d.cin_pad = L.dtype_code(dtype), g.C, g.Cin, sw.cin_pad
        d.H_in, d.W_in, d.k, d.stride, d.pad = g.H_in, g.W_in, g.k, g.stride, g.pad
        d.ph, d.pw, d.dim_head, d.num_blocks, d.eps = g.ph, g.pw, g.dim_head, g.num_blocks, float(g.eps)
        d.inp_u8, d.h_raw, d.w_raw = int(inp_u8), h_raw, w_raw
        d.conv_w, d.ln_w, d.ln_b = p(sw.conv_w), p(sw.ln_w), p(sw.ln_b)
        d.blocks = ctypes.cast(self.blocks, ctypes.POINTER(RvtBlockWeights))
        d.lstm_w, d.lstm_b, d.lstm_wn, d.lstm_bn = p(sw.lstm_w), p(sw.lstm_b), p(sw.lstm_wn), p(sw.lstm_bn)
        self.desc, self.sw, self.g, self.dtype, self.train = d, sw, g, dtype, train
        self._ws_bytes, self._ws_gen = {}, tuning.generation

    def ws_bytes(self, T: int, B: int) -> int:
        """rvt_stage_seq_fwd_ws_bytes, cached by what it depends on: (T, B) and the tuning record (this object outlives a tuning change)."""
        if self._ws_gen != tuning.generation:
            self._ws_bytes, self._ws_gen = {}, tuning.generation
        n = self._ws_bytes.get((T, B))
        if n is None:
            n = self._ws_bytes[(T, B)] = int(L.get_lib().rvt_stage_seq_fwd_ws_bytes(ctypes.byref(self.desc), T, B))
        return n


def plan(call: StageCall, T: int, B: int, save: bool, token_mask) -> RvtStageRoutes:
    """The routes of one stage forward (and of its backward when save)."""
    sw = call.sw
    r = RvtStageRoutes()
    lib = L.get_lib()
    L.check('rvt_stage_routes', lib.rvt_stage_routes(ctypes.byref(call.desc), T, B, int(save), int(sw.dws is not None), int(token_mask is not None),
                                                     ctypes.byref(r)), lib)
    r.conv_dgrad4 = int(r.conv_dgrad4 and sw.conv_wd4 is not None)      # (the packed weight copy exists only for stages with an input gradient)
    return r


def stage_seq_fwd(call: StageCall, inp: torch.Tensor, h0: Optional[torch.Tensor], c0: Optional[torch.Tensor], T: int, B: int) \
        -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (Hall (T+1,B,H,W,C) in the compute dtype — slot 0 scratch, slots 1..T = h_t —, c_last (B,H,W,C) fp32)."""
    g, dt, dev = call.g, call.dtype, inp.device
    lib = L.get_lib()
    st, ws = L.workspace('fwd', inp, call.ws_bytes(T, B), torch.uint8)
    Hall = torch.empty((T + 1, B, g.H, g.W, g.C), dtype=dt, device=dev)
    c_last = torch.empty((B, g.H, g.W, g.C), dtype=torch.float32, device=dev)
    if h0 is not None:
        assert h0.dtype == dt and h0.is_contiguous() and c0 is not None and c0.dtype == torch.float32 and c0.is_contiguous()
    rc = lib.rvt_stage_seq_fwd(ctypes.byref(call.desc), L.ptr(inp), L.ptr(h0), L.ptr(c0), L.ptr(Hall), L.ptr(c_last), L.ptr(ws),
                               ws.numel(), T, B, st)
    L.check('rvt_stage_seq_fwd', rc, lib)
    return Hall, c_last


class LstmBuffers:
    """The ConvLSTM-side buffers of one stage forward, allocated by route for the host loop (rvt_amd/stage.py) and train_forward alike:
    Hall (T+1,B,H,W,C), slot 0 = incoming h (zeros for None); c_last fp32, handed to the caller; scan routes when save: Csave, gates
    (routes 2 / 3; route 3 in the kernel's dump order) and c0_saved - the incoming cell state may alias the caller's tensor (RNNStates
    resets states in place, modules/utils/detection.py:96-113) and BPTT needs the value the forward saw; per-step route: Call, all T+1
    cell states for BPTT or the two a no-grad forward ping-pongs between (c_last = the slot its last step writes), gates when save.
    direct0: the no-grad host loop reads the incoming states where they are at step 0, slot 0 stays unwritten."""

    def __init__(self, r: RvtStageRoutes, g, dt: torch.dtype, dev, T: int, B: int, h0, c0, save: bool, direct0: bool = False):
        from . import ops
        E = lambda *shape, dtype=dt: torch.empty(shape, dtype=dtype, device=dev)
        st, lr = (B, g.H, g.W), r.lstm_route
        self.Hall = E(T + 1, *st, g.C)
        self.Csave = self.gates = self.Call = self.c0_saved = None
        if lr == 0:
            self.Call = E(T + 1 if save else 2, *st, g.C, dtype=torch.float32)
            self.gates = E(T, *st, 4 * g.C) if save else None
        elif save:
            rows = (ops.lstm_scan3_rows(g.C, B * g.H * g.W, r.lstm_scan3_rb),) if lr == 3 else st
            self.Csave, self.gates = E(T, *rows, g.C), (E(T, *rows, 4 * g.C) if lr != 1 else None)
            self.c0_saved = None if c0 is None else c0.clone()
        for buf, s0 in ((self.Hall, h0), (self.Call, c0)):
            if buf is not None and h0 is None:
                buf[0].zero_()                                                    # rnn.py:43-47
            elif buf is not None and not direct0:
                buf[0].copy_(s0)
        self.c_last = self.Call[T % 2] if (lr == 0 and not save) else E(*st, g.C, dtype=torch.float32)

    def fill_saved(self, sv, x: torch.Tensor, x_lstm: Optional[torch.Tensor] = None, hconv: Optional[torch.Tensor] = None) -> None:
        """x: the stage's last block output; x_lstm / hconv: what the DWS-ConvLSTM of the host loop fed the cell instead."""
        sv.x_last, sv.Hall, sv.Call, sv.gates = x, self.Hall, self.Call, self.gates
        sv.xin_lstm, sv.hconv, sv.Csave, sv.c0 = (x if x_lstm is None else x_lstm), hconv, self.Csave, self.c0_saved


# ---- training-side driver (round 6; include/rvt_hip.h: rvt_stage_seq_train_fwd / rvt_stage_seq_bwd, csrc/capi_train.hip) ----------------
# plan() decides the routes; the host owns every tensor that outlives a call; the library sequences the launches.  `StageSaved` is filled
# exactly as the Python host loop fills it, so either backward can consume it.
class TrainTables:
    """What the training driver's records hold for as long as a weight set lives, filled once by header field name
    (weights.ModelWeights._build_grads): the RvtBlockTrain host array - the W^T arena views of `sw.blocks` and the accumulators of the
    gradient records `sg.blocks` - and an RvtStageTrain `template` with `tb`, the stage-level weight copies and the stage record's
    accumulators.  Every forward starts its own RvtStageTrain from the template; the block array is shared."""

    def __init__(self, sw, sg):
        self.tb = (RvtBlockTrain * max(len(sg.blocks), 1))()
        for b, bw, gb in zip(self.tb, (bw for pair in sw.blocks for bw in pair), sg.blocks):
            for k in fields(RvtBlockTrain):
                setattr(b, k, L.ptr(getattr(gb, k) if k.startswith('d_') else bw[k]))
        t = self.template = RvtStageTrain()
        t.struct_bytes = ctypes.sizeof(RvtStageTrain)
        t.tb = ctypes.cast(self.tb, ctypes.POINTER(RvtBlockTrain))
        for k in fields(RvtStageTrain):
            if k.startswith('d_'):
                setattr(t, k, L.ptr(getattr(sg.stage, k)))
        t.lstm_wt, t.conv_wd4, t.conv_wd = L.ptr(sw.lstm_wt), L.ptr(sw.conv_wd4), L.ptr(sw.conv_wd)


class TrainCall:
    """Everything one stage's training forward built for its backward: the descriptor, its own RvtStageTrain (a copy of the weight
    set's template, which keeps the shared block table alive through `call.train`) and RvtBlockSaved array, the routes taken."""
    __slots__ = ('call', 'tr', 'saved_arr', 'inp', 'keep')


def train_forward(call: StageCall, routes: RvtStageRoutes, inp: torch.Tensor, h0, c0, T: int, B: int):
    """Training forward of one stage in ONE library call.  Returns (Hall, c_last, StageSaved) like stage.stage_seq_forward."""
    from .stage import StageSaved
    sw, g = call.sw, call.g
    dt, dev = sw.conv_w.dtype, inp.device
    H, W, C = g.H, g.W, g.C
    F_ = T * B
    E = lambda *shape, dtype=dt: torch.empty(shape, dtype=dtype, device=dev)
    tr = RvtStageTrain.from_buffer_copy(call.train.template)
    tr.routes = routes
    sv = StageSaved()
    sv.routes = routes
    y0, x0 = E(F_, H, W, C), E(F_, H, W, C)
    sv.inp, sv.y0, sv.mask = inp, y0, None
    nb = 2 * g.num_blocks
    saved_arr = (RvtBlockSaved * max(nb, 1))()
    x = x0
    i = 0
    for pair in sw.blocks:
        for bw in pair:
            has_n1 = bw['n1_w'] is not None
            s = dict(xin=x, qkv=None, a=E(F_, H, W, C), xmid=E(F_, H, W, C), hg=None, hgp=None, u=None, v2=None, hpre=False)
            if not routes.attn_block:
                s['qkv'] = E(F_, H, W, 3 * C)
                s['u'] = E(F_, H, W, C) if has_n1 else x
            if routes.mlp_route == 0:
                s['v2'], s['hg'], s['hgp'] = E(F_, H, W, C), E(F_, H, W, 4 * C), E(F_, H, W, 4 * C)
            xout = E(F_, H, W, C)
            b = saved_arr[i]
            b.xin, b.a, b.xmid, b.xout = L.ptr(x), L.ptr(s['a']), L.ptr(s['xmid']), L.ptr(xout)
            b.qkv, b.u = L.ptr(s['qkv']), (L.ptr(s['u']) if (has_n1 and not routes.attn_block) else None)
            b.v2, b.hg, b.hgp = L.ptr(s['v2']), L.ptr(s['hg']), L.ptr(s['hgp'])
            sv.blocks.append(s)
            x = xout
            i += 1
    lb = LstmBuffers(routes, g, dt, dev, T, B, h0, c0, save=True)
    lr = routes.lstm_route
    if lr == 3:
        tr.lstm_wp3 = L.ptr(sw.scan3_packed(bwd=False))
    tr.saved = ctypes.cast(saved_arr, ctypes.POINTER(RvtBlockSaved))
    tr.y0, tr.x0, tr.Hall, tr.c_last = L.ptr(y0), L.ptr(x0), L.ptr(lb.Hall), L.ptr(lb.c_last)
    tr.Csave, tr.gates, tr.Call = L.ptr(lb.Csave), L.ptr(lb.gates), L.ptr(lb.Call)
    lib = L.get_lib()
    rc = lib.rvt_stage_seq_train_fwd(ctypes.byref(call.desc), ctypes.byref(tr), L.ptr(inp), L.ptr(c0) if lr != 0 else None, T, B, L.stream_of(inp))
    L.check('rvt_stage_seq_train_fwd', rc, lib)
    lb.fill_saved(sv, x)
    tc = TrainCall()
    tc.call, tc.tr, tc.saved_arr, tc.inp, tc.keep = call, tr, saved_arr, inp, (y0, x0)
    sv.train = tc
    return lb.Hall, lb.c_last, sv  # (per-step route: c_last was copied out of Call[T] by the library, BPTT keeps the T+1-slot array)


def train_backward(sv, dH, dc_last, T: int, B: int, need_input_grad: bool, prev_cot):
    """BPTT backward of one stage in ONE library call.  Returns (d_input or None, dh0, dc0) like stage.stage_seq_backward."""
    tc = sv.train
    tr, call = tc.tr, tc.call
    sw, g = call.sw, call.g
    dt, dev = sv.y0.dtype, sv.y0.device
    H, W, C = g.H, g.W, g.C
    tr.c0_saved = L.ptr(sv.c0)
    if tr.routes.lstm_route == 3:
        tr.lstm_wtp3 = L.ptr(sw.scan3_packed(bwd=True))
    if dH is None and tr.routes.lstm_route == 0:
        dH = torch.zeros((T, B, H, W, C), dtype=dt, device=dev)
    dcl = None if dc_last is None else dc_last.to(torch.float32).contiguous()
    dh0 = torch.empty((B, H, W, C), dtype=dt, device=dev)
    dc0 = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
    d_in = torch.empty((T * B, g.H_in, g.W_in, g.Cin), dtype=dt, device=dev) if need_input_grad else None
    lib = L.get_lib()
    st, ws = L.workspace('train', sv.y0, int(lib.rvt_stage_seq_bwd_ws_bytes(ctypes.byref(call.desc), ctypes.byref(tr), T, B)), torch.uint8)
    rc = lib.rvt_stage_seq_bwd(ctypes.byref(call.desc), ctypes.byref(tr), L.ptr(tc.inp), L.ptr(dH), L.ptr(dcl), L.ptr(prev_cot), L.ptr(d_in),
                               L.ptr(dh0), L.ptr(dc0), L.ptr(ws), ws.numel(), T, B, st)
    L.check('rvt_stage_seq_bwd', rc, lib)
    return d_in, dh0, dc0
