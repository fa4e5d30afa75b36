"""Rounding models of the bf16 fused kernels: the YARDSTICK of the ceilings in tests/bounds.py (idiom of tests/test_optim.py and
tests/test_bnact.py: fp64 truth, and a yardstick that is not the code under test).

Each function restates one fused operation in plain torch on the CPU - always the CPU, so that the `emu` and the `hip` id of a test
get the same yardstick - in fp32 arithmetic, and rounds to bf16 exactly where the kernel converts fp32 to bf16: a stored output, a
saved tensor, or an MFMA operand built from an accumulator.  Nowhere else.  It takes the bf16 inputs the test hands to the kernel.
What it returns are the values BEFORE the final storage rounding (the ceiling adds one bf16 ulp for outputs stored in bf16).

`rounding=False, dtype=torch.float64` switches every rounding point off; the result must then equal the test's fp64 autograd truth
to 1e-9 relative (`pin`, asserted once per case as tests/test_bnact.py `_Case.__init__` does), which pins the model's MATHEMATICS:
only its rounding can differ from the truth.

The backward passes are written out (no autograd): several kernels round a PRODUCT inside a reduction (the LayerNorm parameter
gradients go through an MFMA against an identity operand, so du * xhat and du are converted to bf16 before they are summed), and the
attention backward recomputes q / k / v with other bias placements than the forward - neither is a rounding of an autograd edge.  The
forward roundings are what `t + (t.bfloat16().float() - t).detach()` would be and the gradient roundings what an identity Function
with a rounding backward would be; written out they are just `_r(t)`.

ROUNDING POINTS (kernel file : line of the conversion)

mlp_half - LN -> fc1 -> GELU -> fc2 * gamma + residual
    v2 = LN2(x), fc1 operand and saved tensor    mlp.hpp:215  ln_pieces.hpp:46 (forward, dgrad)  mlp_chain.hpp:363 (wgrad / both)  mlp_stream.hpp:654
    g = GELU(pre), fc2 operand and saved tensor  mlp.hpp:272  mlp_chain.hpp:96 :394  mlp_stream.hpp:164 :705;  mlp.hpp:746 (recompute)
    gp = GELU'(pre), saved (`saved_gp`)          mlp.hpp:278 - rvt_mlp_bwd_dgrad multiplies by the STORED value (mlp.hpp:450)
    (W2 gamma)^T, rounded by the host            rvt_amd/weights.py; the tests build it the same way
    dh = dg * GELU'(pre), fc1-dgrad / dW1 operand, stored by rvt_mlp_bwd_dgrad      mlp.hpp:453 :747  mlp_chain.hpp:191 :395  mlp_stream.hpp:420 :706
        (db1 sums the UNROUNDED products: mlp_chain.hpp:392, mlp_stream.hpp:704, mlp.hpp:744)
    dv2 = dh W1 through a bf16 tile (`dv2_bf16`: rvt_mlp_bwd_recompute_both only)   mlp_chain.hpp:445
    dv2 * xhat and dv2 before the column sums (`dln_bf16`: the chain / streamed input-gradient kernels)   mlp_chain.hpp:227-228  mlp_stream.hpp:494-495
        (mlp.hpp:502 :786 and mlp_chain.hpp:465-466 sum in fp32)
    stored outputs y, pre, dxmid: returned before their rounding (mlp.hpp:308 :280 :510 :794, mlp_chain.hpp:124 :242 :471, mlp_stream.hpp:220 :521)

attn_half - [LN ->] qkv -> softmax(Q K^T) V -> proj * gamma + residual       (attn_block.hpp; acc_to_frags / arr_slot_frag convert)
    u = LN1(x), qkv operand (and the `u` output of the backward)ln_pieces.hpp:95
    forward  q (+ bias), k (NO bias: softmax is invariant to it), v (NO bias: added to the output, rows of P sum to 1)   :156 :163 :166
             the UN-normalised exp(scale (s - max)) as the P V operand        :182
             a = P V / sum + bv, proj operand and saved tensor                :190 :197;   xmid stored :227
    backward q (+ bias), k (no bias), v (+ bias)                              :401 :409 :381 :387 :384
             dO = dxmid (Wp gamma), (Wp gamma)^T rounded by the host          :404 :412
             P = softmax in fp32 (normalised), dS = P (dP - delta) scale, both as MFMA operands   :441-442 :450
             dq, dk, dv: stored and the operand of du = dqkv Wqkv             :360 :363
             LN / PRE: du * xhat and du before the column sums                :516-517;   dx stored :532 :540
    `handover_bf16` is the two-launch route the PRE kernel replaces: dx = dxmid + du stored in bf16 (:540), then ln_bwd_kernel
    (rowops.hpp:54-111: fp32 sums of the bf16 rows).

attn_core - softmax(Q K^T) V on a saved qkv tensor: q, k, v, dO are the stored bf16 values, no bias anywhere    (attn_core2.hpp; the
    helpers of acc_frags.hpp :30-42 and opm.hpp :96-105 convert; the transposes by identity MFMA, :22-29, are exact)
    forward  the UN-normalised exp(scale (s - max)) as the P V operand        :92 (staged :180);   out stored :101 (staged :189)
    backward P = softmax in fp32 (normalised, :272 / :415) through the LDS tile for dV          :281 (staged :424)
             dS = P (dP - delta) scale through the LDS tile for dK, from the registers for dQ   :282 :289 (staged :425 :432)
             dq, dk, dv stored                                                :245 (staged :384)
    `_softmax_bwd` is this backward and that of attn_half: the two kernels differ in where q, k, v, dO come from, not in the softmax.

lstm - ConvLSTM cell with a 1x1 conv, T steps, and its BPTT.  z = [x | h] W^T + b accumulates in fp32, the gates and c_t stay fp32.
    h_t rounded where it is stored; the stored value is the next step's operand (`h_bf16`)
             gemm.hpp:634 (per step)  lstm_scan.hpp:187  lstm_scan2.hpp:202 (s2_pack)  lstm_scan3.hpp:172
    c_t copy for the backward (`c`, returned before its rounding)    lstm_scan.hpp:188  lstm_scan2.hpp:213  lstm_scan3.hpp:181;  c_last stays fp32
    activated gates saved for the backward (`gates`, before rounding)  gemm.hpp:637-640  lstm_scan.hpp:190-193 (W_REG)  lstm_scan3.hpp:177-180
    backward, `saved_gates`: f, i, o, g read back from that save      rowops.hpp:239-242  lstm_scan.hpp:433-436 (GATES)  lstm_scan3.hpp:286-289
             off: recomputed in fp32 from x_t and the stored h_{t-1}  lstm_scan.hpp:438-441  lstm_scan2.hpp:492-495
    backward, `c_bf16`: c_{t-1} from the bf16 save, the incoming fp32 c0 converted the same way, tanh(c_t) of f c_{t-1} + i g rebuilt from it
             lstm_scan.hpp:309-310 :443 :445  lstm_scan2.hpp:444 :455 :498  lstm_scan3.hpp:291 :296 :304
             off: c_t and c_{t-1} are the forward's fp32 tensors      rowops.hpp:245-246 :249
    `dz_bf16`: dz, the operand of [dx | dh] = dz W and of dW = dz^T [x | h], and a stored output
             rowops.hpp:258-261  lstm_scan.hpp:449-452  lstm_scan2.hpp:510-511  lstm_scan3.hpp:306-309
    `db_bf16`: db from the rounded dz - lstm_scan2.hpp:361 :384 (product against ones), and every test that sums the stored dz itself;
             off: lstm_scan.hpp:453 sums the fp32 values
    dx_t stored (lstm_scan.hpp:502, lstm_scan2.hpp:589, lstm_scan3.hpp:348); dh_{t-1} and dc stay in fp32 registers across the steps
    (lstm_scan.hpp:503, lstm_scan2.hpp:586, lstm_scan3.hpp:349); dh0 stored, dc0 fp32.

dgrad_ln - dx = add + LN'(dy W; x) and, `inside`, dx = LN'(dy W + add; x)     (dgrad_ln.hpp)
    du (+ add) rounded "as the two-launch chain stores it"                    :186 - AFTER the row sums s1 / s2 took the fp32 values (:182-184)
    du * xhat before the column sums (du itself is already bf16)              :246-247;   dx stored :215
    `fused=False` is the chain it replaces: du stored by the GEMM epilogue, then ln_bwd_kernel on the bf16 rows (rowops.hpp:54-111).

ln_linear - u = LN(x) is the GEMM operand and the saved tensor (ln_linear.hpp:107-115, layernorm_fwd rowops.hpp:50); y stored (:134).

linear_ep - y = epilogue(x W^T): the linear entry points on BOTH GEMM engines.  fp32 accumulation of bf16 products everywhere.
    `gelu_in`: GELU(x) is converted to bf16 on its way into the operand tile           gemm.hpp:190 (xf_apply, XfGelu; 128-row engine only)
    128-row engine (gemm.hpp): the side tensor is combined with the fp32 accumulator, ONE rounding at the store
             EpStore v + bias + add :419-420   EpScaleRes res + gamma (v + bias) :461-462   EpMul v * mul :515-516
             EpGeluBwd v * GELU'(pre) :479-480   EpGeluDual g, gp :496-498   EpDgradScatter v + add :588-589
    256-wide engine (ppgemm.hpp), `side_rounded`: `convert` rounds c1 (acc + c0) into the LDS scratch                      :312-316 :334
             and `store_rows` adds / multiplies the bf16 side tensor to the ROUNDED value and rounds a second time          :350-351
             (PP_SCALE_RES: res + bf16(gamma (v + bias));  PP_ADD: bf16(v + bias) + add;  PP_MUL: bf16(v) * mul).  PP_STORE and
             PP_GELU_DUAL have no side tensor: one rounding (:334).  The conv input gradient by 2 x 2 blocks (rvt_conv_dgrad4) with an
             added cotangent is PP_ADD and rounds twice as well; the parity-class route (EpDgradScatter) rounds once.
wgrad - dW = dy^T x, column sums of dy: fp32 throughout (split-K partial tiles and their fold, ppgemm_tn.hpp); `gelu_in` as above (gemm.hpp:190).
layernorm - rowops.hpp ln_fwd_kernel / ln_bwd_kernel: two-pass statistics in fp32; y stored :45, dx (+ dres) stored :108; dw, db are
    fp32 sums of fp32 products (:100).  No interior rounding point.
conv_fwd / conv_dgrad / conv_wgrad - im2col products on the same engines: no interior rounding point but `side_rounded` above.
    `scale` / `shift` / `act` (rvt_conv_bn_act_fwd): act(fma(acc, scale, shift)) on the fp32 accumulator, one store    gemm.hpp:439-442
stem - y0 = conv of the uint8 planes (exact in bf16), stored stem.hpp:218; the LayerNorm statistics and output are taken from the
    STORED y0 (:219 converts it back, "the statistics see what the backward will see"), x stored :246: the test models LN(y0) by
    `layernorm` on the kernel's own y0.  stem_wgrad: `conv_wgrad`, fp32.
dwconv - rowops.hpp dwconv_kernel: bias + nine fp32 products, one store :327; dwconv_wgrad_kernel: fp32 sums.
lin_gelu_ws - fc1 + GELU on the weight-stationary kernel (ln_linear.hpp lin_gelu_ws_kernel): pre = x W^T + b in fp32; Phi and GELU' are
    READ AT THE NEAREST POINT of the table of gelu_lut.hpp (`snap`): index = round((pre + X) N / 2X) clamped to [0, N]      gelu_lut.hpp:90-94
             g = pre * Phi(snapped pre) with the UNSNAPPED pre as the factor, gp = GELU'(snapped pre)                     gelu_lut.hpp:123
             both stored ln_linear.hpp:258-259.  Not a bf16 conversion but a quantisation of the argument, |error| <= 5.8e-4 on GELU'.
"""
import math

import torch
import torch.nn.functional as F


def _r(t, on=True):
    """One fp32 -> bf16 conversion (round to nearest even, what v_cvt_pk_bf16_f32 and the emulator's cast do)."""
    return t.bfloat16().to(t.dtype) if on else t


def _prep(dtype, *ts):
    return [None if t is None else t.detach().to('cpu', dtype) for t in ts]


def _ln(x, eps):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    return d * rstd, rstd


def _ln_bwd(d, xhat, rstd, w, stats_from=None):
    """rstd (d w - mean(d w) - xhat mean(d w xhat)); `stats_from`: the tensor the two row means are taken from (dgrad_ln.hpp:182)."""
    gs = (d if stats_from is None else stats_from) * w
    m1 = gs.mean(-1, keepdim=True)
    m2 = (gs * xhat).mean(-1, keepdim=True)
    return rstd * (d * w - m1 - xhat * m2)


def _gelu_both(x):
    phi = 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    return x * phi, phi + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def pin(model64, truth, what):
    """The model with its rounding off, in fp64, IS the test's fp64 truth (1e-9 relative to the tensor's max)."""
    for k, want in truth.items():
        got, want = model64[k], want.detach().double().cpu()
        assert got.shape == want.shape, (what, k, got.shape, want.shape)
        err, s = (got - want).abs().max().item(), max(want.abs().max().item(), 1.0)
        assert err <= 1e-9 * s, f'{what}: model (rounding off, fp64) vs fp64 truth, {k}: {err:.3e} of {s:.3e}'


# ------------------------------------------------------------------------------------------------------------------- MLP half
def mlp_half(x, lw, lb, w1, b1, w2, b2, gam, dy=None, eps=1e-5, *, rounding=True, dtype=torch.float32, saved_gp=False,
             dln_bf16=False, dv2_bf16=False):
    """x [M][C], w1 [4C][C], w2 [C][4C], dy [M][C] -> dict of v2, pre, g, gp, y and (dy given) dh, dxmid, dln_w, dln_b, dW1, db1,
    S2, cs2.  S2 = dy^T g and cs2 = colsum(dy) are the raw fc2 products (gamma is applied by the LayerScale fold)."""
    x, lw, lb, w1, b1, w2, b2, gam, dy = _prep(dtype, x, lw, lb, w1, b1, w2, b2, gam, dy)
    r = lambda t: _r(t, rounding)
    xhat, rstd = _ln(x, eps)
    v2 = xhat * lw + lb
    v2r = r(v2)
    pre = v2r @ w1.t() + b1
    g, gp = _gelu_both(pre)
    gr = r(g)
    y = x + gam * (gr @ w2.t() + (b2 if b2 is not None else 0.0))
    out = dict(v2=v2, pre=pre, g=g, gp=gp, y=y)
    if dy is None:
        return out
    w2g = r(w2 * gam[:, None])
    dh = (dy @ w2g) * (r(gp) if saved_gp else gp)
    dhr = r(dh)
    dv2 = dhr @ w1
    if dv2_bf16:
        dv2 = r(dv2)
    out.update(dh=dh, dxmid=dy + _ln_bwd(dv2, xhat, rstd, lw),
               dln_w=(r(dv2 * xhat) if dln_bf16 else dv2 * xhat).sum(0), dln_b=(r(dv2) if dln_bf16 else dv2).sum(0),
               dW1=dhr.t() @ v2r, db1=dh.sum(0), S2=dy.t() @ gr, cs2=dy.sum(0))
    return out


# ------------------------------------------------------------------------------------------------------------- attention half
def _to_parts(x, Fr, H, W, ph, pw, window):
    """(F, H, W, c) -> (partitions, ph * pw, c): windows (maxvit.py:273-287) or the dilated grid (:290-304)."""
    c = x.shape[-1]
    if window:
        t = x.reshape(Fr, H // ph, ph, W // pw, pw, c).permute(0, 1, 3, 2, 4, 5)
    else:
        t = x.reshape(Fr, ph, H // ph, pw, W // pw, c).permute(0, 2, 4, 1, 3, 5)
    return t.reshape(-1, ph * pw, c)


def _from_parts(t, Fr, H, W, ph, pw, window):
    c = t.shape[-1]
    t = t.reshape(Fr, H // ph, W // pw, ph, pw, c)
    t = t.permute(0, 1, 3, 2, 4, 5) if window else t.permute(0, 3, 1, 4, 2, 5)
    return t.reshape(Fr, H, W, c)


def _split_heads(qkv, heads, dh):
    """(partitions, L, 3C) with the channels of a head as [q | k | v] (maxvit.py:347) -> [3][partitions][heads][L][dh]."""
    return qkv.reshape(qkv.shape[0], qkv.shape[1], heads, 3, dh).permute(3, 0, 2, 1, 4)


def _softmax_bwd(q, k, v, dO, scale, r):
    """q, k, v, dO [partitions][heads][L][dh] -> dqkv (partitions, L, 3C): P = softmax(scale Q K^T) in fp32 (normalised),
    dS = P (dP - delta) scale; P and dS are MFMA operands (`r`), the three products accumulate in fp32."""
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    dp = dO @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * scale
    pr, dsr = r(p), r(ds)
    dq, dk, dv = dsr @ k, dsr.transpose(-1, -2) @ q, pr.transpose(-1, -2) @ dO
    NP, heads, L, dh = q.shape
    return torch.stack([dq, dk, dv], 0).permute(1, 3, 2, 0, 4).reshape(NP, L, 3 * heads * dh)


def attn_core(qkv, dout, geom, *, rounding=True, dtype=torch.float32):
    """The attention core on a saved qkv tensor (rvt_attn_fwd / rvt_attn_bwd): qkv (F, H, W, 3C) with the biases already in it, dout
    (F, H, W, C) or None; geom = (F, H, W, C, dim_head, ph, pw, window) -> dict of out and (dout given) dqkv.  q, k, v and dO are the
    bf16 tensors as stored: the only conversions are the softmax operands."""
    Fr, H, W, C, dh, ph, pw, window = geom
    heads, scale = C // dh, dh ** -0.5
    qkv, dout = _prep(dtype, qkv, dout)
    r = lambda t: _r(t, rounding)
    part = lambda t: _to_parts(t.reshape(Fr, H, W, -1), Fr, H, W, ph, pw, window)
    back = lambda t: _from_parts(t, Fr, H, W, ph, pw, window)
    q, k, v = _split_heads(part(qkv), heads, dh)
    NP, L = q.shape[0], q.shape[2]
    s = (q @ k.transpose(-1, -2)) * scale
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (r(e) @ v) / e.sum(-1, keepdim=True)
    out = dict(out=back(o.permute(0, 2, 1, 3).reshape(NP, L, C)))
    if dout is not None:
        dO = part(dout).reshape(NP, L, heads, dh).permute(0, 2, 1, 3)
        out['dqkv'] = back(_softmax_bwd(q, k, v, dO, scale, r))
    return out


def attn_half(x, ln_w, ln_b, wqkv, bqkv, wp, bp, gamma, wpg_t, dxm, geom, eps=1e-5, *, y0=None, rounding=True, dtype=torch.float32,
              handover_bf16=False):
    """geom = (F, H, W, C, dim_head, ph, pw, window).  ln_w None: no norm1.  y0 given (with ln_w = the weight of the norm in FRONT
    of the block, ln_b unused): the PRE form, x = the block input as stored, dy0 = LN'(dxmid + du; y0).  The backward multiplies
    dxmid by wpg_t^T = the host-rounded (Wp gamma) when rounding, by gamma * wp (what autograd does) when not.
    -> dict of u, a, xmid, dqkv, dx (PRE: dy0), dln_w, dln_b."""
    Fr, H, W, C, dh, ph, pw, window = geom
    heads, scale = C // dh, dh ** -0.5
    x, ln_w, ln_b, wqkv, bqkv, wp, bp, gamma, wpg_t, dxm, y0 = _prep(dtype, x, ln_w, ln_b, wqkv, bqkv, wp, bp, gamma, wpg_t, dxm, y0)
    r = lambda t: _r(t, rounding)
    part = lambda t: _to_parts(t.reshape(Fr, H, W, -1), Fr, H, W, ph, pw, window)
    back = lambda t: _from_parts(t, Fr, H, W, ph, pw, window)
    pre = y0 is not None
    xt = part(x)
    out = {}
    if ln_w is not None and not pre:
        xhat, rstd = _ln(xt, eps)
        u = xhat * ln_w + ln_b
        out['u'] = back(u)
        ur = r(u)
    else:
        ur = xt
    NP, L = xt.shape[0], xt.shape[1]
    qkv = _split_heads(ur @ wqkv.t(), heads, dh)                                         # [3][NP][heads][L][dh], no bias yet
    bq, _, bv = bqkv.reshape(heads, 3, dh).permute(1, 0, 2)[:, None, :, None, :]        # [3] x [1][heads][1][dh]; the k bias is dropped
    # ---- forward (attn_block_fwd_kernel)
    q, k, v = r(qkv[0] + bq), r(qkv[1]), r(qkv[2])
    s = (q @ k.transpose(-1, -2)) * scale
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    a = (r(e) @ v) / e.sum(-1, keepdim=True) + bv
    a = a.permute(0, 2, 1, 3).reshape(NP, L, C)
    out['a'] = back(a)
    out['xmid'] = back(xt + gamma * (r(a) @ wp.t() + bp))
    if dxm is None:
        return out
    # ---- backward (attn_block_bwd_kernel): everything recomputed from the block input
    dt_ = part(dxm)
    wpg = wpg_t.t() if rounding else gamma[:, None] * wp                                 # [c][a]
    dO = r(dt_ @ wpg).reshape(NP, L, heads, dh).permute(0, 2, 1, 3)
    dqkv = _softmax_bwd(r(qkv[0] + bq), r(qkv[1]), r(qkv[2] + bv), dO, scale, r)
    out['dqkv'] = back(dqkv)
    du = r(dqkv) @ wqkv
    if pre or ln_w is not None:
        if pre:
            xhat, rstd = _ln(part(y0), eps)
            d = du + dt_
            if handover_bf16:
                d = r(d)
            res = 0.0
        else:
            d, res = du, dt_
        rr = (lambda t: t) if handover_bf16 else r
        out.update(dx=back(res + _ln_bwd(d, xhat, rstd, ln_w)), dln_w=rr(d * xhat).sum((0, 1)), dln_b=rr(d).sum((0, 1)))
    else:
        out['dx'] = back(dt_ + du)
    return out


# ------------------------------------------------------------------------------------------------------ LN + linear family
def ln_linear(x, lw, lb, w, b, eps=1e-5, *, rounding=True, dtype=torch.float32):
    """u = LN(x), y = u W^T + b  (w [N][C]) -> dict of u, y."""
    x, lw, lb, w, b = _prep(dtype, x, lw, lb, w, b)
    xhat, _ = _ln(x, eps)
    u = xhat * lw + lb
    return dict(u=u, y=_r(u, rounding) @ w.t() + b)


def linear(x, w, b=None, *, rounding=True, dtype=torch.float32):
    """y = x W^T + b: fp32 accumulation of the bf16 products, nothing rounded before the store (`rounding` has nothing to switch)."""
    x, w, b = _prep(dtype, x, w, b)
    return dict(y=x @ w.t() + (b if b is not None else 0.0))


def linear_ep(x, w, b=None, *, gelu_in=False, gamma=None, res=None, add=None, mul=None, gelu_pre=None, dual=False, side_rounded=False,
              rounding=True, dtype=torch.float32):
    """The linear entry points with their epilogues, x [M][K], w [N][K] -> dict of y, or (dual) of g = GELU(x W^T + b), gp = GELU'.
      gamma, res   y = res + gamma (x W^T + b)          add   y = x W^T + b + add
      mul          y = (x W^T) * mul                    gelu_pre   y = (x W^T) * GELU'(gelu_pre)
    gelu_in: the operand is bf16(GELU(x)).  side_rounded: the 256-wide engine - gamma (v + b), v + b or v is rounded to bf16 BEFORE
    res / add / mul is combined with it (ppgemm.hpp:334 then :350); off: the 128-row engine combines in fp32."""
    x, w, b, gamma, res, add, mul, gelu_pre = _prep(dtype, x, w, b, gamma, res, add, mul, gelu_pre)
    assert (res is not None) + (add is not None) + (mul is not None) + (gelu_pre is not None) + bool(dual) <= 1 and (gamma is None) == (res is None)
    r = lambda t: _r(t, rounding)
    rs = r if side_rounded else (lambda t: t)
    if gelu_in:
        x = r(_gelu_both(x)[0])
    v = x @ w.t() + (b if b is not None else 0.0)
    if dual:
        g, gp = _gelu_both(v)
        return dict(g=g, gp=gp)
    if res is not None:
        return dict(y=res + rs(gamma * v))
    if add is not None:
        return dict(y=rs(v) + add)
    if mul is not None:
        return dict(y=rs(v) * mul)
    if gelu_pre is not None:
        return dict(y=v * _gelu_both(gelu_pre)[1])
    return dict(y=v)


def wgrad(dy, x, *, gelu_in=False, rounding=True, dtype=torch.float32):
    """dW = dy^T x and the column sums of dy, both kept in fp32 (gemm.hpp split-K, ppgemm_tn.hpp): no rounding point but the GELU'd
    operand (`gelu_in`: x -> bf16(GELU(x)), gemm.hpp:190).  `+=` into an fp32 buffer: the caller scales the model."""
    dy, x = _prep(dtype, dy, x)
    if gelu_in:
        x = _r(_gelu_both(x)[0], rounding)
    return dict(dW=dy.t() @ x, colsum=dy.sum(0))


def layernorm(x, w, b, dy=None, dres=None, eps=1e-5, *, rounding=True, dtype=torch.float32):
    """rowops.hpp ln_fwd_kernel / ln_bwd_kernel: x [rows][C] -> dict of y and (dy given) dx = LN'(dy; x) + dres, dw, db.  Two-pass
    statistics, everything in fp32, nothing rounded before the stores (`rounding` has nothing to switch)."""
    x, w, b, dy, dres = _prep(dtype, x, w, b, dy, dres)
    xhat, rstd = _ln(x, eps)
    out = dict(y=xhat * w + (b if b is not None else 0.0))
    if dy is not None:
        out.update(dx=_ln_bwd(dy, xhat, rstd, w) + (dres if dres is not None else 0.0), dw=(dy * xhat).sum(0), db=dy.sum(0))
    return out


GELU_NLUT_N, GELU_LUT_X = 8192, 6.0        # gelu_lut.hpp: "read at the NEAREST of 8192 points" of [-X, X], X = 6


def lin_gelu_ws(x, w, b, *, rounding=True, dtype=torch.float32):
    """fc1 + GELU on the weight-stationary kernel: pre = x W^T + b -> dict of g, gp.  Phi and GELU' are read at the nearest of the
    N + 1 = 8193 grid points -X + (2X / N) i, N = 8192, X = 6 (gelu_lut.hpp, comment of the nearest-entry tables); the factor of
    g = pre * Phi(snapped pre) is the unsnapped pre.  `rounding` switches the snapping (the model's only quantisation) off."""
    x, w, b = _prep(dtype, x, w, b)
    pre = x @ w.t() + b
    xs = pre
    if rounding:
        s = GELU_NLUT_N / (2.0 * GELU_LUT_X)
        xs = torch.round((pre + GELU_LUT_X) * s).clamp(0.0, float(GELU_NLUT_N)) / s - GELU_LUT_X
    phi = 0.5 * (1.0 + torch.erf(xs * (1.0 / math.sqrt(2.0))))
    return dict(g=pre * phi, gp=_gelu_both(xs)[1])


def dgrad_ln(dy, w, x, add, lw, eps=1e-5, *, inside=False, fused=True, rounding=True, dtype=torch.float32):
    """dy [M][K], w [K][C], x [M][C] = the LayerNorm input, add [M][C] or None -> dict of dx, dln_w, dln_b.
    inside: the added cotangent enters the norm (rvt_linear_dgrad_preln).  fused = False: the two launches (GEMM epilogue stores
    du [+ add] in bf16, ln_bwd_kernel reads it back)."""
    dy, w, x, add, lw = _prep(dtype, dy, w, x, add, lw)
    r = lambda t: _r(t, rounding)
    xhat, rstd = _ln(x, eps)
    du = dy @ w
    res = 0.0
    if add is not None:
        if inside:
            du = du + add
        else:
            res = add
    dur = r(du)
    if fused:
        return dict(dx=res + _ln_bwd(dur, xhat, rstd, lw, stats_from=du), dln_w=r(dur * xhat).sum(0), dln_b=dur.sum(0))
    return dict(dx=res + _ln_bwd(dur, xhat, rstd, lw), dln_w=(dur * xhat).sum(0), dln_b=dur.sum(0))


# --------------------------------------------------------------------------------------------------------------- ConvLSTM
def lstm(x, h0, c0, w, b, dH=None, dc_last=None, *, rounding=True, dtype=torch.float32, saved_gates=False, c_bf16=True,
         dz_bf16=True, h_bf16=True, db_bf16=False):
    """The 1x1-conv ConvLSTM (rnn.py:52-67) over T steps and its BPTT.  x [T][M][C], h0 [M][C], c0 [M][C] or None (zeros), w [4C][2C]
    in the natural gate order f, i, o, g and input order [x | h], b [4C]; dH [T][M][C] and dc_last [M][C] (None = zeros).
    -> dict of h, c [T][M][C], c_last, gates [T][M][4C] and (dH or dc_last given) dz [T][M][4C], dx, dh0, dc0, dW, db.
    What differs between the kernels:
      saved_gates  the backward reads the activated gates from the forward's bf16 save instead of recomputing them in fp32
      c_bf16       the backward reads c_{t-1} as bf16 (Csave; the incoming fp32 c0 is converted the same way) and rebuilds
                   c_t = f c_{t-1} + i g from it; off: both cell states are the forward's fp32 tensors (per-step kernels)
      dz_bf16      dz is the bf16 operand of [dx | dh] = dz W and of dW = dz^T [x | h]
      h_bf16       h_t is rounded where it is stored, and the stored value is the next step's operand
      db_bf16      db sums the ROUNDED dz (a product against ones, or the test's own sum of the stored dz) instead of the fp32 values"""
    x, h0, c0, w, b, dH, dc_last = _prep(dtype, x, h0, c0, w, b, dH, dc_last)
    r = lambda t: _r(t, rounding)
    T, M, C = x.shape
    c = torch.zeros(M, C, dtype=dtype) if c0 is None else c0
    c_in, h = c, h0
    hs, cs, gs, hin = [], [], [], []
    for t in range(T):
        hin.append(h)
        z = torch.cat([x[t], h], -1) @ w.t() + b
        f, i, o, g = torch.sigmoid(z[:, :C]), torch.sigmoid(z[:, C:2 * C]), torch.sigmoid(z[:, 2 * C:3 * C]), torch.tanh(z[:, 3 * C:])
        c = f * c + i * g
        hn = o * torch.tanh(c)
        hs.append(hn)
        cs.append(c)
        gs.append(torch.cat([f, i, o, g], -1))
        h = r(hn) if h_bf16 else hn
    out = dict(h=torch.stack(hs), c=torch.stack(cs), c_last=c, gates=torch.stack(gs))
    if dH is None and dc_last is None:
        return out
    dh_rec = torch.zeros(M, C, dtype=dtype)
    dc_rec = torch.zeros(M, C, dtype=dtype) if dc_last is None else dc_last
    dzs, dxs = [None] * T, [None] * T
    dW, db = torch.zeros_like(w), torch.zeros_like(b)
    for t in range(T - 1, -1, -1):
        f, i, o, g = (r(gs[t]) if saved_gates else gs[t]).split(C, -1)
        cp = cs[t - 1] if t > 0 else c_in
        if c_bf16:
            cp = r(cp)
            cn = f * cp + i * g
        else:
            cn = cs[t]
        dh = dh_rec if dH is None else dH[t] + dh_rec
        tc = torch.tanh(cn)
        dc = dc_rec + dh * o * (1.0 - tc * tc)
        dz = torch.cat([dc * cp * f * (1.0 - f), dc * g * i * (1.0 - i), dh * tc * o * (1.0 - o), dc * i * (1.0 - g * g)], -1)
        dc_rec = dc * f
        dzr = r(dz) if dz_bf16 else dz
        dxh = dzr @ w
        dxs[t], dh_rec, dzs[t] = dxh[:, :C], dxh[:, C:], dz
        dW = dW + dzr.t() @ torch.cat([x[t], hin[t]], -1)
        db = db + (r(dz) if db_bf16 else dz).sum(0)
    out.update(dz=torch.stack(dzs), dx=torch.stack(dxs), dh0=dh_rec, dc0=dc_rec, dW=dW, db=db)
    return out


def _silu(z):
    return z * torch.sigmoid(z)


def conv_fwd(x, w, stride, pad, scale=None, shift=None, act=0, *, rounding=True, dtype=torch.float32):
    """x (F, H, W, Cin) channels-last, w (Cout, Cin, k, k) -> y (F, Ho, Wo, Cout); as `linear`, no interior rounding point.
    scale / shift / act (rvt_conv_bn_act_fwd): the affine on the fp32 accumulator, then SiLU (act = 1), one store."""
    x, w, scale, shift = _prep(dtype, x, w, scale, shift)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, None, stride, pad).permute(0, 2, 3, 1)
    if scale is not None:
        y = y * scale + shift
        if act:
            y = _silu(y)
    return dict(y=y)


def conv_dgrad(dy, w, stride, pad, H, W, add=None, *, side_rounded=False, rounding=True, dtype=torch.float32):
    """Input gradient of conv_fwd: dy (F, Ho, Wo, Cout), w (Cout, Cin, k, k) -> dx (F, H, W, Cin) (+ add).  side_rounded: the 2 x 2-block
    route with an added cotangent (ppgemm.hpp PP_ADD) rounds the product before it adds; the parity-class route adds in fp32."""
    dy, w, add = _prep(dtype, dy, w, add)
    dx = torch.nn.grad.conv2d_input((dy.shape[0], w.shape[1], H, W), w, dy.permute(0, 3, 1, 2).contiguous(), stride, pad).permute(0, 2, 3, 1)
    if add is not None:
        dx = (_r(dx, rounding) if side_rounded else dx) + add
    return dict(dx=dx)


def conv_wgrad(x, dy, k, stride, pad, *, rounding=True, dtype=torch.float32):
    """dW (Cout, Cin, k, k) = the weight gradient of conv_fwd, kept in fp32 on both engines (split-K im2col, ppgemm_tn.hpp CONV)."""
    x, dy = _prep(dtype, x, dy)
    size = (dy.shape[-1], x.shape[-1], k, k)
    return dict(dW=torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).contiguous(), size, dy.permute(0, 3, 1, 2).contiguous(), stride, pad))


def dwconv(x, w, b, dy=None, *, rounding=True, dtype=torch.float32):
    """Depth-wise 3 x 3 (rowops.hpp): x, dy (N, H, W, C), w (C, 9), b (C) -> dict of y and (dy given) dx, dw (C, 9), db; fp32, one store."""
    x, w, b, dy = _prep(dtype, x, w, b, dy)
    C = x.shape[-1]
    w4, xc = w.reshape(C, 1, 3, 3), x.permute(0, 3, 1, 2).contiguous()
    out = dict(y=F.conv2d(xc, w4, b, padding=1, groups=C).permute(0, 2, 3, 1))
    if dy is not None:
        dc = dy.permute(0, 3, 1, 2).contiguous()
        out.update(dx=torch.nn.grad.conv2d_input(xc.shape, w4, dc, 1, 1, 1, C).permute(0, 2, 3, 1),
                   dw=torch.nn.grad.conv2d_weight(xc, w4.shape, dc, 1, 1, 1, C).reshape(C, 9), db=dy.sum((0, 1, 2)))
    return out
