"""The optimizer step on the device: value clip + AdamW + OneCycleLR in one launch (csrc/optim.hpp, rvt_optim_step).

Mirror of the reference's optimisation contract (modules/detection.py:360-392 `configure_optimizers`, config/general.yaml
`training`, and the trainer's `gradient_clip_val` with `gradient_clip_algorithm='value'`): per step, clip every gradient to
[-clip, clip], run `torch.optim.AdamW` (decoupled weight decay, no amsgrad), advance a linear two-phase `OneCycleLR`.

  * `AdamW(params, lr, betas, eps, weight_decay, clip_value=None, schedule=None)`: a `torch.optim.Optimizer` with parameter
    groups (own lr / betas / eps / weight_decay each).  `step()` is ONE `rvt_optim_step` call for every parameter of every
    group and nothing else on the device: no allocation, no host synchronisation, capturable in a hipGraph.  The step count
    lives on the device and the call advances it, so a replayed graph walks the schedule with nothing written by the host.
  * `OneCycle(total_steps, pct_start, div_factor, final_div_factor)`: the schedule with the REFERENCE's reading of
    final_div_factor (final lr = max lr / final_div_factor), converted to torch's the way detection.py:374 does.
    A group's `lr` is the schedule's maximum, as in the reference (`max_lr=lr`).
  * `from_train_config(params, training_cfg)`: the optimizer the reference's `training` config section describes.

Differences to the torch pieces a caller can see: the STORED gradients are not clipped (the clamp happens on the way into the
update; `clip_grad_value_` rewrites them); one counter drives the bias correction and the schedule position of every
parameter (torch counts per parameter: a parameter that gets its first gradient late starts at 1 there, at the common count
here); past the schedule's last step the learning rate stays at its final value (torch raises); `group['lr']` is never
rewritten by the schedule (`current_lr()` reads the device counter and evaluates it, for logging).  `state_dict()` /
`load_state_dict()` speak `torch.optim.AdamW`'s format in both directions (a Lightning checkpoint's `optimizer_states[0]`
loads; our state loads into torch); these and `current_lr()` are the only members that read the device back.  There is no
PyTorch fallback: a missing kernel raises.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L

Tensor = torch.Tensor

CHUNK = L.ENUMS['RVT_OPTIM_CHUNK_ELEMS']              # elements per row of the chunk table (include/rvt_hip.h: RvtOptimChunk)
SCHEDULE = ('lr_init', 'lr_max', 'lr_final', 'warm_end', 'last')      # the schedule fields of RvtOptimGroup = OneCycle.constants()


class OneCycle:
    """Linear two-phase one-cycle schedule, the reference's parameters (config/general.yaml: lr_scheduler):
    initial lr = max lr / div_factor, final lr = max lr / final_div_factor."""

    def __init__(self, total_steps: int, pct_start: float = 0.3, div_factor: float = 25.0, final_div_factor: float = 1e4):
        if int(total_steps) != total_steps or total_steps <= 0:
            raise ValueError(f'total_steps must be a positive integer, got {total_steps}')
        if not 0.0 <= pct_start <= 1.0:
            raise ValueError(f'pct_start must be in [0, 1], got {pct_start}')
        if div_factor <= 0 or final_div_factor <= 0:
            raise ValueError('div_factor and final_div_factor must be positive')
        self.total_steps, self.pct_start = int(total_steps), float(pct_start)
        self.div_factor, self.final_div_factor = float(div_factor), float(final_div_factor)

    @property
    def torch_final_div_factor(self) -> float:
        """What torch.optim.lr_scheduler.OneCycleLR takes as final_div_factor (it divides the INITIAL lr): detection.py:374."""
        return self.final_div_factor / self.div_factor

    def constants(self, max_lr: float) -> Tuple[float, float, float, float, float]:
        """(lr_init, lr_max, lr_final, warm_end, last) of the group table, computed the way OneCycleLR.__init__ does."""
        lr_init = max_lr / self.div_factor
        lr_final = lr_init / self.torch_final_div_factor
        return lr_init, float(max_lr), lr_final, float(self.pct_start * self.total_steps) - 1, float(self.total_steps - 1)


def schedule_lr(lr_init: float, lr_max: float, lr_final: float, warm_end: float, last: float, pos: float) -> float:
    """Host restatement of optim_lr (csrc/optim.hpp): the learning rate at schedule position pos, in double."""
    if pos <= warm_end:
        return (lr_max - lr_init) * (pos / warm_end) + lr_init if warm_end > 0.0 else lr_max
    if pos <= last:
        return (lr_final - lr_max) * ((pos - warm_end) / (last - warm_end)) + lr_max
    return lr_final


def _check_grad(p: Tensor, g: Tensor) -> None:
    if g.is_sparse:
        raise RuntimeError('rvt_amd.optim.AdamW does not support sparse gradients')
    if g.dtype != torch.float32:
        raise TypeError(f'rvt_amd.optim.AdamW needs float32 gradients, got {g.dtype}')
    if g.device != p.device or not g.is_contiguous() or g.numel() != p.numel():
        raise ValueError('gradients must be dense, contiguous and on the device of their parameter')


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, clip_value: Optional[float] = None, schedule: Optional[OneCycle] = None,
                 amsgrad: bool = False, maximize: bool = False):
        if clip_value is not None and not clip_value >= 0:
            raise ValueError(f'clip_value must be None or >= 0, got {clip_value}')
        if schedule is not None and not isinstance(schedule, OneCycle):
            raise TypeError('schedule must be an rvt_amd.optim.OneCycle or None')
        self.clip_value, self.schedule = clip_value, schedule
        self.max_blocks = 0                               # grid cap of the launch (0 = the library's; tests: grid-stride walks)
        self._sealed = False
        # torch.optim.AdamW's group keys, so that state_dict() loads there and its state_dict() loads here
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._sealed = True
        self._check_groups()
        ps = [p for g in self.param_groups for p in g['params']]
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32:
                raise TypeError(f'rvt_amd.optim.AdamW updates float32 parameters, got {p.dtype}')
            if p.device != dev:
                raise ValueError(f'all parameters must live on one device, got {dev} and {p.device}')
            if p.is_sparse or not p.is_contiguous():
                raise ValueError('rvt_amd.optim.AdamW needs dense contiguous parameters')
        # the two moments: one flat arena each, every view 16-byte aligned
        off, spans = 0, []
        for p in ps:
            spans.append((off, p.numel()))
            off += (p.numel() + 3) // 4 * 4
        self._exp_avg = torch.zeros(max(off, 4), dtype=torch.float32, device=dev)
        self._exp_avg_sq = torch.zeros(max(off, 4), dtype=torch.float32, device=dev)
        self._views: Dict[Tensor, Tuple[Tensor, Tensor]] = {
            p: (self._exp_avg[o:o + n].view(p.shape), self._exp_avg_sq[o:o + n].view(p.shape)) for p, (o, n) in zip(ps, spans)}
        self._step = torch.zeros(1, dtype=torch.int64, device=dev)        # optimizer steps done so far; the kernel advances it
        self._chunks: Optional[L.DeviceTable] = None
        self._groups: Optional[L.DeviceTable] = None
        self._sig = self._hyper = None

    # ---- construction-time checks ---------------------------------------------------------------------------
    def add_param_group(self, param_group: Dict[str, Any]) -> None:
        if self._sealed:
            raise NotImplementedError('rvt_amd.optim.AdamW sizes its state arenas at construction: pass every group to __init__')
        super().add_param_group(param_group)

    def _check_groups(self) -> None:
        for g in self.param_groups:
            if g.get('amsgrad', False):
                raise ValueError('rvt_amd.optim.AdamW does not implement amsgrad')
            if g.get('maximize', False):
                raise ValueError('rvt_amd.optim.AdamW does not implement maximize')
            b1, b2 = g['betas']
            if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and g['eps'] >= 0.0 and g['lr'] >= 0.0 and g['weight_decay'] >= 0.0):
                raise ValueError(f'invalid hyper-parameters lr={g["lr"]} betas={g["betas"]} eps={g["eps"]} '
                                 f'weight_decay={g["weight_decay"]}')

    # ---- tables -----------------------------------------------------------------------------------------------
    def _group_rows(self) -> List[Dict[str, float]]:
        """One RvtOptimGroup per parameter group, by field name."""
        clip = -1.0 if self.clip_value is None else float(self.clip_value)
        rows = []
        for g in self.param_groups:
            lr = float(g['lr'])
            sched = self.schedule.constants(lr) if self.schedule is not None else (lr, lr, lr, 0.0, 0.0)
            rows.append(dict(zip(SCHEDULE, sched), beta1=float(g['betas'][0]), beta2=float(g['betas'][1]), eps=float(g['eps']),
                             weight_decay=float(g['weight_decay']), clip=clip))
        return rows

    def _build_chunks(self, entries) -> L.DeviceTable:
        parts = []
        for p, g, gi in entries:
            m, v = self._views[p]
            if p not in self.state or 'exp_avg' not in self.state[p]:
                self.state[p]['exp_avg'], self.state[p]['exp_avg_sq'] = m, v
            n = p.numel()
            arr = np.zeros((n + CHUNK - 1) // CHUNK, dtype=L.row_dtype('RvtOptimChunk'))
            o = np.arange(len(arr), dtype=np.uint64) * np.uint64(4 * CHUNK)
            arr['p'], arr['g'], arr['m'], arr['v'] = p.data_ptr() + o, g.data_ptr() + o, m.data_ptr() + o, v.data_ptr() + o
            arr['n'] = np.minimum(n - np.arange(len(arr), dtype=np.int64) * CHUNK, CHUNK)
            arr['group'] = gi
            parts.append(arr)
        return L.DeviceTable('RvtOptimChunk').upload(self._step.device, np.concatenate(parts))

    # ---- the step ---------------------------------------------------------------------------------------------
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        entries = []
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                _check_grad(p, g)
                entries.append((p, g, gi))
        if not entries:
            return loss
        sig = tuple((p.data_ptr(), g.data_ptr(), gi) for p, g, gi in entries)
        if sig != self._sig:                              # (with the models' zero_copy_grads: never again after the first step)
            self._chunks = self._build_chunks(entries)
            self._sig = sig
        if len(self._chunks) == 0:                        # (only empty tensors)
            return loss
        rows = self._group_rows()
        if rows != self._hyper:
            self._check_groups()
            self._groups = L.DeviceTable('RvtOptimGroup')
            for row in rows:
                self._groups.add(**row)
            self._groups.upload(self._step.device)
            self._hyper = rows
        L.call('rvt_optim_step', L.ptr(self._chunks.dev), len(self._chunks), L.ptr(self._groups.dev), len(self._groups),
               L.ptr(self._step), int(self.max_blocks), L.stream_of(self._step))
        # the kernel wrote through raw pointers: tell autograd and the models' weight caches (backbone / FPN / head re-pack their
        # kernel-side copies when a parameter's version moves).  Host-side counters only, no device work.
        torch.autograd.graph.increment_version([p for p, _, _ in entries])
        return loss

    # ---- what reads the device back ---------------------------------------------------------------------------
    def step_count(self) -> int:
        return int(self._step.item())

    def current_lr(self) -> List[float]:
        """Learning rate of every group at the NEXT step (the schedule at position = steps done).  Reads the step count back."""
        k = self.step_count()
        return [schedule_lr(*(row[f] for f in SCHEDULE), float(k)) for row in self._group_rows()]

    def state_dict(self) -> Dict[str, Any]:
        k = self.step_count()
        for st in self.state.values():
            if 'exp_avg' in st:
                st['step'] = torch.tensor(float(k), dtype=torch.float32)
        sd = super().state_dict()
        if self.schedule is not None:                     # the keys OneCycleLR keeps in the groups; lr = the current one, as there
            for g, row in zip(sd['param_groups'], self._group_rows()):
                g.update(lr=schedule_lr(*(row[f] for f in SCHEDULE), float(k)), initial_lr=row['lr_init'], max_lr=row['lr_max'],
                         min_lr=row['lr_final'])
        return sd

    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        steps = sorted({float(st['step']) for st in state_dict['state'].values() if 'step' in st})
        if len(steps) > 1:
            raise ValueError(f'the per-parameter step entries disagree ({steps[0]:g} .. {steps[-1]:g}): one counter drives the bias '
                             f'correction and the schedule of every parameter here')
        k = steps[0] if steps else 0.0
        if k < 0 or k != int(k):
            raise ValueError(f'step = {k} is not a step count')
        for g in state_dict['param_groups']:
            if g.get('amsgrad', False) or g.get('maximize', False):
                raise ValueError('rvt_amd.optim.AdamW implements neither amsgrad nor maximize')
        peaks = [g['lr'] for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, peak in zip(self.param_groups, peaks):
            init, mx = g.pop('initial_lr', None), g.pop('max_lr', None)
            g.pop('min_lr', None)
            if self.schedule is not None:
                # a scheduled optimizer's `lr` is the CURRENT rate: the maximum is max_lr where the checkpoint has one
                g['lr'] = mx if mx is not None else (init * self.schedule.div_factor if init is not None else peak)
        self._check_groups()
        for p, (m, v) in self._views.items():
            st = self.state.get(p)
            if st and 'exp_avg' in st:
                m.copy_(st['exp_avg'])
                v.copy_(st['exp_avg_sq'])
                self.state[p] = {'exp_avg': m, 'exp_avg_sq': v}
            else:
                m.zero_()
                v.zero_()
                self.state.pop(p, None)
        self._step.fill_(int(k))
        self._sig = self._hyper = None


def _key(cfg, name: str, default=None):
    if isinstance(cfg, dict):
        return cfg.get(name, default)
    try:
        return cfg[name]
    except (KeyError, TypeError, AttributeError):
        return getattr(cfg, name, default)


def from_train_config(params, training_cfg) -> AdamW:
    """The optimizer of the reference's `training` config section (config/general.yaml; modules/detection.py:360-392):
    learning_rate, weight_decay, gradient_clip_val (by value; None or 0 = off) and lr_scheduler.{use, total_steps, pct_start,
    div_factor, final_div_factor}.  training_cfg: a dict, an AttrDict or an OmegaConf node."""
    clip = _key(training_cfg, 'gradient_clip_val')
    clip = float(clip) if clip is not None and clip > 0 else None
    sp = _key(training_cfg, 'lr_scheduler')
    schedule = None
    if sp is not None and _key(sp, 'use', False):
        total = _key(sp, 'total_steps')
        if total is None or total <= 0:
            raise ValueError('lr_scheduler.total_steps must be a positive integer when lr_scheduler.use is set')
        schedule = OneCycle(total, _key(sp, 'pct_start'), _key(sp, 'div_factor'), _key(sp, 'final_div_factor'))
    return AdamW(params, lr=_key(training_cfg, 'learning_rate'), weight_decay=_key(training_cfg, 'weight_decay'), clip_value=clip,
                 schedule=schedule)
