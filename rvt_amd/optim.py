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
  * `AdamW.attach_monitor(named_parameters, ring, skip_nonfinite) -> GradMonitor` (opt-in; csrc/gradstats.hpp, rvt_grad_stats):
    per-tensor gradient statistics into a device ring (the reference's GradFlowLogCallback without a host round trip) and a
    non-finite verdict that `step()` then obeys on the device (rvt_optim_step_guarded: the GradScaler's step-skip of
    `precision: 16`).  Without a monitor, or with skip_nonfinite=False, `step()` is `rvt_optim_step` as before.

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

import ctypes
import math
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L

Tensor = torch.Tensor

CHUNK = L.ENUMS['RVT_OPTIM_CHUNK_ELEMS']              # elements per row of the chunk table (include/rvt_hip.h: RvtOptimChunk)
MAX_SCALARS = L.ENUMS['RVT_GRADSTAT_MAX_SCALARS']     # scalars per observation (include/rvt_hip.h: RvtGradStatHead)
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
        self._monitor: Optional['GradMonitor'] = None     # attach_monitor()

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
    def _entries(self) -> List[Tuple[Tensor, Tensor, int]]:
        """(parameter, gradient, group index) of every parameter that has a gradient, in group order."""
        entries = []
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                _check_grad(p, g)
                entries.append((p, g, gi))
        return entries

    def _sync_chunks(self, entries) -> None:
        """The chunk table of these entries: rebuilt when an address or the set of gradients moved, and the monitor's chunk-to-tensor
        array with it, in the same place, so the two cannot drift apart."""
        sig = tuple((p.data_ptr(), g.data_ptr(), gi) for p, g, gi in entries)
        if sig != self._sig:                              # (with the models' zero_copy_grads: never again after the first step)
            self._chunks = self._build_chunks(entries)
            self._sig = sig
            if self._monitor is not None:
                self._monitor._rebuild(entries)

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        entries = self._entries()
        if not entries:
            return loss
        self._sync_chunks(entries)
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
        mon = self._monitor
        if mon is not None and mon.skip_nonfinite:        # the step that obeys the monitor's latest verdict
            L.call('rvt_optim_step_guarded', L.ptr(self._chunks.dev), len(self._chunks), L.ptr(self._groups.dev), len(self._groups),
                   L.ptr(self._step), L.ptr(mon._verdict), int(self.max_blocks), L.stream_of(self._step))
        else:
            L.call('rvt_optim_step', L.ptr(self._chunks.dev), len(self._chunks), L.ptr(self._groups.dev), len(self._groups),
                   L.ptr(self._step), int(self.max_blocks), L.stream_of(self._step))
        # the kernel wrote through raw pointers: tell autograd and the models' weight caches (backbone / FPN / head re-pack their
        # kernel-side copies when a parameter's version moves).  Host-side counters only, no device work.  (A step the guard dropped
        # on the device bumps them too: the host does not look.)
        torch.autograd.graph.increment_version([p for p, _, _ in entries])
        return loss

    def attach_monitor(self, named_parameters, ring: int = 64, skip_nonfinite: bool = True) -> 'GradMonitor':
        """Gradient statistics and the non-finite guard (GradMonitor below).  named_parameters: (name, parameter) pairs, e.g.
        `model.named_parameters()`; every parameter must be one of this optimizer's.  With skip_nonfinite, step() becomes
        rvt_optim_step_guarded and obeys the verdict of the latest observe().  A second call replaces the monitor."""
        mon = GradMonitor(self, named_parameters, ring, skip_nonfinite)
        self._monitor = mon
        self._sig = None                                  # both tables are rebuilt together at the next observe() / step()
        return mon

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


class GradMonitor:
    """Per-tensor gradient statistics and the non-finite verdict, computed on the device over the optimizer's own chunk table
    (csrc/gradstats.hpp, rvt_grad_stats) into a ring the host reads later.  Made by `AdamW.attach_monitor`.

    What it replaces in the reference's loop: `GradFlowLogCallback` (callbacks/gradflow.py; `param.grad.abs().mean()` per named
    parameter = one host synchronisation each) and the GradScaler of `precision: 16`, which drops a step whose gradients hold an
    inf or a NaN.  `observe()` is one library call (two launches), allocates nothing, does not synchronise and is capturable; it
    writes slot `step % ring`, with `step` the optimizer's device counter read on the device, and the verdict that
    `AdamW.step()` obeys when skip_nonfinite is set.  Call it after the backward and, under data parallelism, after the gradient
    reduction has finished: every rank then sees the same gradients and reaches the same verdict with no collective added.  Call
    it before every step: the guarded step obeys the LATEST verdict, however old.

    A skipped step advances neither the bias correction nor the schedule position, because one device counter drives both
    (Lightning would still step the scheduler); the next observation therefore lands in the same ring slot and replaces the
    skipped one: `skipped_steps()` is the record that it happened.  `read()`, `grad_flow()` and `skipped_steps()` are the only
    members that read the device back.  When the set of gradients or an address changes, the optimizer rebuilds its chunk table
    and this monitor's chunk-to-tensor array with it, and the ring starts empty again (its rows are indexed by table position)."""

    def __init__(self, opt: AdamW, named_parameters, ring: int, skip_nonfinite: bool):
        if isinstance(ring, bool) or int(ring) != ring or ring < 1:
            raise ValueError(f'ring must be a positive integer, got {ring}')
        own = {id(p) for g in opt.param_groups for p in g['params']}
        self._named: List[Tuple[str, Tensor]] = []
        for name, p in named_parameters:
            if id(p) not in own:
                raise ValueError(f'parameter {name!r} is not one of the optimizer\'s')
            self._named.append((str(name), p))
        self._name_of = {id(p): name for name, p in self._named}
        self.opt, self.ring, self.skip_nonfinite = opt, int(ring), bool(skip_nonfinite)
        dev = opt._step.device
        self._cap = max(len(own), 1)                      # rows per slot: one per tensor of the chunk table, at most every parameter
        self._head_dt, self._stat_dt = L.row_dtype('RvtGradStatHead'), L.row_dtype('RvtGradStat')
        hb, sb = self.ring * self._head_dt.itemsize, self.ring * self._cap * self._stat_dt.itemsize
        # one device buffer = one copy per read(): [ring] heads | [ring][cap] rows | verdict[2]
        self._buf = torch.zeros(hb + sb + 16, dtype=torch.uint8, device=dev)
        self._heads, self._stats = self._buf[:hb], self._buf[hb:hb + sb]
        self._verdict = self._buf[hb + sb:].view(torch.int64)
        self._host: Optional[Tensor] = None
        self._pending = None                              # (event or None,) of a copy read() has started and not yet parsed
        self._first: Optional[Tensor] = None              # int32 [n_tensors + 1] first-chunk indices, on the device
        self._rows: List[Optional[str]] = []              # name (None: not among named_parameters) of each tensor of the table
        self._numel: List[int] = []
        self._ws_bytes = 0
        self._scalars: Tuple[Tensor, ...] = ()
        self._empty_ring()

    # ---- tables -----------------------------------------------------------------------------------------------
    def _empty_ring(self) -> None:
        heads = np.zeros(self.ring, dtype=self._head_dt)
        heads['step'] = -1                                # no observation in this slot
        self._heads.copy_(torch.from_numpy(heads.view(np.uint8).reshape(-1)))

    def _rebuild(self, entries) -> None:
        """Called by the optimizer exactly when it rebuilds its chunk table: the tensors of the table in table order."""
        tensors = [p for p, _, _ in entries if p.numel() > 0]
        counts = [(p.numel() + CHUNK - 1) // CHUNK for p in tensors]
        first = np.zeros(len(tensors) + 1, dtype=np.int32)
        first[1:] = np.cumsum(counts)
        self._first = torch.from_numpy(first).to(self._buf.device)
        self._rows = [self._name_of.get(id(p)) for p in tensors]
        self._numel = [p.numel() for p in tensors]
        self._ws_bytes = int(L.get_lib().rvt_grad_stats_ws_bytes(int(first[-1])))
        self._pending = None
        self._empty_ring()

    # ---- the observation --------------------------------------------------------------------------------------
    def observe(self, scalars=()) -> None:
        """rvt_grad_stats on the current gradients.  scalars: up to RVT_GRADSTAT_MAX_SCALARS one-element float32 tensors on the
        optimizer's device (the loss terms, ...); the launch reads their values and stores them in the slot's head, which is how a
        loss reaches the host without an `.item()` per step.  A parameter whose `.grad` is None is left out, as in the reference."""
        scalars = tuple(scalars)
        if len(scalars) > MAX_SCALARS:
            raise ValueError(f'at most {MAX_SCALARS} scalars per observation, got {len(scalars)}')
        dev = self._buf.device
        for t in scalars:
            if not isinstance(t, Tensor) or t.dtype != torch.float32:
                raise TypeError(f'scalars must be float32 tensors, got {t.dtype if isinstance(t, Tensor) else type(t).__name__}')
            if t.numel() != 1 or t.device != dev:
                raise ValueError(f'scalars must be one-element tensors on {dev}')
        opt = self.opt
        entries = opt._entries()
        if not entries:
            return
        opt._sync_chunks(entries)
        if len(opt._chunks) == 0:
            return
        st, ws = L.workspace('gradstats', opt._step, self._ws_bytes, torch.uint8)
        ptrs = (ctypes.c_void_p * len(scalars))(*[L.ptr(t) for t in scalars]) if scalars else None
        self._scalars = scalars                           # (a captured graph keeps reading these addresses)
        L.call('rvt_grad_stats', L.ptr(opt._chunks.dev), len(opt._chunks), L.ptr(self._first), len(self._rows), L.ptr(opt._step),
               ptrs, len(scalars), L.ptr(self._stats), self._cap, L.ptr(self._heads), self.ring, L.ptr(self._verdict), L.ptr(ws),
               ws.numel(), int(opt.max_blocks), st)

    # ---- what reads the device back ---------------------------------------------------------------------------
    def read(self, last: int = 1, wait: bool = True) -> Optional[List[Dict[str, Any]]]:
        """The `last` most recent observations in the ring, oldest first.  ONE non-blocking copy of the ring into a pinned buffer
        plus an event; wait=False returns None while that copy is still in flight (ask again: the same copy is picked up).
        Per observation: step (optimizer steps done before it), scalars, global_grad_norm, grad_abs_max, nonfinite, and `params`:
        name -> grad_abs_mean (abs_sum / numel), grad_norm, grad_abs_max, param_norm, nonfinite, and the raw figures they come from
        (numel, grad_abs_sum, grad_sq_sum, param_sq_sum; grad_sq_sum of the head too).  The sums run over the finite elements only."""
        if last < 1:
            raise ValueError(f'last must be at least 1, got {last}')
        if self._pending is None:
            if self._host is None:
                self._host = torch.empty(self._buf.numel(), dtype=torch.uint8, pin_memory=self._buf.is_cuda)
            self._host.copy_(self._buf, non_blocking=True)
            ev = None
            if self._buf.is_cuda:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self._buf.device))
            self._pending = (ev,)
        ev = self._pending[0]
        if ev is not None:
            if wait:
                ev.synchronize()
            elif not ev.query():
                return None
        self._pending = None
        raw = self._host.numpy()
        hb, sb = self._heads.numel(), self._stats.numel()
        heads = raw[:hb].view(self._head_dt)
        stats = raw[hb:hb + sb].view(self._stat_dt).reshape(self.ring, self._cap)
        slots = sorted((int(heads['step'][s]), s) for s in range(self.ring) if heads['step'][s] >= 0)[-last:]
        out = []
        for k, s in slots:
            h = heads[s]
            params = {}
            for t, (name, n) in enumerate(zip(self._rows, self._numel)):
                r = stats[s, t]
                if name is None or r['nonfinite'] < 0:
                    continue
                params[name] = dict(grad_abs_mean=float(r['abs_sum']) / n, grad_norm=math.sqrt(float(r['sq_sum'])),
                                    grad_abs_max=float(r['abs_max']), param_norm=math.sqrt(float(r['param_sq_sum'])),
                                    nonfinite=int(r['nonfinite']), numel=n, grad_abs_sum=float(r['abs_sum']),
                                    grad_sq_sum=float(r['sq_sum']), param_sq_sum=float(r['param_sq_sum']))
            out.append(dict(step=k, scalars=[float(v) for v in h['scalars'][:int(h['n_scalars'])]],
                            global_grad_norm=math.sqrt(float(h['sq_sum'])), grad_abs_max=float(h['abs_max']),
                            nonfinite=int(h['nonfinite']), grad_sq_sum=float(h['sq_sum']), params=params))
        return out

    def skipped_steps(self) -> int:
        """Steps the guarded step() dropped so far.  Reads the device back."""
        return int(self._verdict[1].item())

    def grad_flow(self, slot: int = -1) -> Dict[str, List[Any]]:
        """{'name': [...], 'grad_abs': [...]} of one observation (slot: index into read(last=ring), -1 = the newest), in the order of
        named_parameters: the `data_dict` the reference's get_grad_flow_figure builds (callbacks/utils/visualization.py: every
        parameter with requires_grad and a gradient; the mean of |grad|).  Reads the device back."""
        rec = self.read(last=self.ring)[slot]
        out: Dict[str, List[Any]] = {'name': [], 'grad_abs': []}
        for name, p in self._named:
            if p.requires_grad and name in rec['params']:
                out['name'].append(name)
                out['grad_abs'].append(rec['params'][name]['grad_abs_mean'])
        return out


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
