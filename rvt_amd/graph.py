"""hipGraph capture of a whole optimisation step.

The reference removes its per-op launch overhead with ``torch.compile(mode='reduce-overhead')`` (CUDA graphs under a
tracing compiler; maxvit_rnn.py:43-51).  Here nothing is traced: every kernel behind include/rvt_hip.h takes an explicit
stream, allocates nothing and synchronises nothing, so the step — prepack, weight pack, four stage-major forwards, the
BPTT backward, the gradient fold, (the RCCL all-reduces,) the fused optimizer — is
captured once as it is issued and replayed as ONE graph launch.  The optimizer is torch's fused AdamW (capturable=True) or
rvt_amd.optim.AdamW: gradient clip by value + AdamW + OneCycleLR as one launch of this library, with the step count and therefore
the schedule position on the device, so a replay needs nothing refreshed by the host.  Shapes are static per (T, B, resolution) bucket, which
is how the reference trains (fixed sequence length and batch size, config/experiment/*).

    step = GraphedStep(lambda: train_step(static_batch))     # warm-up runs + capture
    static_batch.copy_(next_batch); step()                   # replay

Inference has two captured forms of the streaming step (T = 1, recurrent state carried on the device): GraphedStreamStep replays the
backbone, GraphedDetectorStream the whole detector - frame in, kept boxes out.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch


class GraphedStep:
    def __init__(self, fn: Callable[[], None], warmup: int = 3, device: Optional[torch.device] = None, models=()):
        """fn must read its inputs from tensors that stay alive and keep their addresses (copy new data INTO them), must
        not synchronise with the host, and should leave parameter gradients in place (rvt_amd assigns persistent bucket
        views to ``.grad``; use ``optimizer.zero_grad(set_to_none=True)`` inside fn)."""
        self.fn = fn
        # models whose kernel-side weight copies the captured step re-packs: a replay updates the parameters without bumping
        # their version counters on the host, so the next inference forward must not trust its cache
        self.models = tuple(models)
        for m in self.models:                    # (checked before anything runs: a capture that fails at its first replay is too late)
            if not all(callable(getattr(m, a, None)) for a in ('invalidate_weight_cache', 'weight_caches')):
                raise TypeError(f'GraphedStep: a {type(m).__name__} has no invalidate_weight_cache() / weight_caches() (rvt_amd modules do)')
        # SIDE EFFECT: the captured step needs stable gradient addresses, so the models switch to zero-copy gradient hand-off
        # (rvt_amd/backbone.py: .grad = persistent bucket views, torch.autograd.grad sees no backbone gradients); close()
        # restores the flags for later eager use of the same modules
        self._saved_flags = [getattr(m, 'zero_copy_grads', False) for m in self.models]
        for m in self.models:
            m.zero_copy_grads = True
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
        for _ in range(max(1, warmup)):          # eager warm-up: sizes every grow-only workspace, the occupancy caches and
            fn()                                 # the optimizer state before anything is recorded
        torch.cuda.synchronize(dev)
        # the capture allocates the step's activations once more, in the graph's private pool: give the eager steps'
        # cached blocks back first (RVT-Base 1 Mpx T=21 B=24 keeps ~110 GiB cached per pool)
        torch.cuda.empty_cache()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            fn()
        # the graph addresses the weight caches the warm-up built (descriptor tables, packed weights, gradient buckets) by raw
        # pointer: they live as long as the graph does.  __call__ drops the MODELS' references after every replay; without these the
        # buffers went back to the allocator and the next tensor allocated between two replays landed on a table the graph reads.
        self._held = [m.weight_caches() for m in self.models]

    def close(self) -> None:
        """Drop the graph and give the models their gradient hand-off mode back (eager use after a captured phase)."""
        self.graph = None
        self._held = []
        for m, f in zip(self.models, self._saved_flags):
            m.zero_copy_grads = f
            for p in m.parameters():
                p.grad = None            # bucket views would be overwritten by the next eager backward
            m.invalidate_weight_cache()

    def __call__(self) -> None:
        self.graph.replay()
        for m in self.models:
            m.invalidate_weight_cache()


class GraphedStreamStep:
    """One streaming-inference step (T = 1, the ConvLSTM state carried from call to call: the validation / deployment loop of
    modules/detection.py:231-255) as ONE hipGraph launch.  A step is ~50 short launches (20 - 250 us each at B = 64); replayed as a
    graph the gaps between them shrink.  The input frame and the recurrent state live in static buffers:

        stream = GraphedStreamStep(model, example_frame)       # eager warm-up + capture (the state starts from zeros)
        feats = stream(frame)                                   # copies `frame` in, replays; feats: {stage: (B, C, H, W)} STATIC tensors
        stream.reset()  /  stream.reset(mask)                   # new sequences: zero the state (of the samples where mask is set)

    The features returned are the graph's own buffers: valid until the next call (copy what has to outlive it).  The parameters must
    not change while the graph lives (inference); call close() before training the model again."""

    def __init__(self, model, example_frame: torch.Tensor, warmup: int = 3):
        assert example_frame.is_cuda and not model.training, 'GraphedStreamStep: an eval-mode model and a CUDA frame (B, C, h, w)'
        self.model = model
        self.x = torch.empty_like(example_frame)
        self.x.copy_(example_frame)
        with torch.no_grad():
            st = None
            for _ in range(max(2, warmup)):                     # eager warm-up: weight pack, workspaces, occupancy caches
                _, st = model(self.x, st)
            # static state buffers (same shapes / strides as the states the model hands back)
            self.states = [tuple(t.clone(memory_format=torch.preserve_format) for t in pair) for pair in st]
            self.reset()
            torch.cuda.synchronize(self.x.device)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                feats, new = model(self.x, self.states)
                for (h, c), (hn, cn) in zip(self.states, new):
                    h.copy_(hn)
                    c.copy_(cn)
            self.feats = feats
        self.reset()

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Zero the recurrent state - of every sample, or of those where the bool mask (B,) is set (modules/utils/detection.py:96-113)."""
        for h, c in self.states:
            if mask is None:
                h.zero_()
                c.zero_()
            else:
                h[mask] = 0
                c[mask] = 0

    def __call__(self, frame: torch.Tensor):
        self.x.copy_(frame)
        self.graph.replay()
        return self.feats

    def close(self) -> None:
        self.graph = None
        self.feats = None


class GraphedDetectorStream:
    """One streaming DETECTION step of an eval-mode rvt_amd.YoloXDetector - masked state reset, backbone (T = 1), PAFPN, the head's
    prediction maps, decode + score filter + NMS (rvt_yolox_detect), state carry - as ONE hipGraph launch with no host
    synchronisation: frame in, the kept boxes out.

        stream = GraphedDetectorStream(detector, example_frame, conf_thre=0.1, nms_thre=0.45)    # eager warm-up + capture
        det, count, anchor_idx = stream(frame)            # copies `frame` into stream.frame_buffer, replays
        builder.build_from_table(table, out=...)          # or: a producer writes stream.frame_buffer in place ...
        det, count, anchor_idx = stream()                 # ... and the step replays on it: no frame copy at all
        stream.reset_mask.copy_(is_first)                 # new sequences: uint8 (B,), applied by the NEXT step on the device
        stream.reset()                                    # every state back to zeros

    `frame_buffer` is the graph's static input, `reset_mask` a static uint8 (B,) device tensor: the captured step zeroes the state rows of
    the samples whose byte is set (rvt_state_reset_masked on every state tensor) before the backbone reads them and clears the mask at
    its end, so marking a sequence boundary is a device-side copy - no boolean index_put, no host synchronisation.  The three tensors
    returned are the graph's own buffers: valid until the next call (clone what has to outlive it).  The parameters must not change
    while the graph lives (inference); call close() before training the detector again."""

    def __init__(self, detector, example_frame: torch.Tensor, conf_thre: float, nms_thre: float, class_agnostic: bool = False,
                 max_det: Optional[int] = None, warmup: int = 3):
        from . import ops
        assert example_frame.is_cuda and not detector.training, 'GraphedDetectorStream: an eval-mode detector and a CUDA frame (B, C, h, w)'
        self.detector = detector
        self.frame_buffer = torch.empty_like(example_frame)
        self.frame_buffer.copy_(example_frame)
        dev = example_frame.device
        self.reset_mask = torch.zeros(example_frame.shape[0], dtype=torch.uint8, device=dev)
        args = (float(conf_thre), float(nms_thre), bool(class_agnostic), max_det)
        with torch.no_grad():
            st = None
            for _ in range(max(2, warmup)):                     # eager warm-up: weight packs, workspaces, occupancy caches
                dets, st = detector.detect(self.frame_buffer, st, *args)
            self.out = tuple(torch.empty_like(t) for t in dets)  # the graph's own outputs, not the per-shape cache other callers share
            # static state buffers (same shapes / strides as the states the detector hands back)
            self.states = [tuple(t.clone(memory_format=torch.preserve_format) for t in pair) for pair in st]
            self.reset()
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                for pair in self.states:
                    for t in pair:                              # (B, C, H, W)-shaped views of channels-last storage
                        ops.state_reset_masked(t.permute(0, 2, 3, 1) if not t.is_contiguous() else t, self.reset_mask)
                _, new = detector.detect(self.frame_buffer, self.states, *args, out=self.out)
                for (h, c), (hn, cn) in zip(self.states, new):
                    h.copy_(hn)
                    c.copy_(cn)
                self.reset_mask.zero_()
        self.reset()

    def reset(self) -> None:
        """Zero the recurrent state of every sample (and forget pending reset marks)."""
        for h, c in self.states:
            h.zero_()
            c.zero_()
        self.reset_mask.zero_()

    def __call__(self, frame: Optional[torch.Tensor] = None):
        if self.graph is None:
            raise RuntimeError('GraphedDetectorStream: the stream was closed (close() dropped its graph); build a new one')
        if frame is not None:
            fb = self.frame_buffer
            if tuple(frame.shape) != tuple(fb.shape) or frame.dtype != fb.dtype:
                raise ValueError(f'GraphedDetectorStream: frame must be {fb.dtype} {tuple(fb.shape)} like frame_buffer, '
                                 f'got {frame.dtype} {tuple(frame.shape)}')
            fb.copy_(frame)
        self.graph.replay()
        return self.out

    def close(self) -> None:
        self.graph = None
        self.out = None
