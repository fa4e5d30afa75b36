"""Spatial training augmentation on the device: horizontal flip, zoom-in and zoom-out of event sequences and their box labels
(csrc/augment.hpp: rvt_augment_planes, rvt_augment_labels).

Mirror of the reference's `RandomSpatialAugmentorGenX` (data/utils/augmentor.py) and of the label transforms it calls
(data/genx_utils/labels.py: flip_lr_, zoom_in_and_rescale_, zoom_out_and_rescale_, scale_).  The reference runs in data-loader
workers, one sequence at a time; here the random draw stays on the host (a few scalars per sample) and the work runs on the
device for the whole batch: one launch for the planes (or one per time step for a list of separately allocated tensors), one
for the labels, no host synchronisation, bit-identical to the reference on recorded fixtures.

  * `RandomSpatialAugmentorGenX(dataset_hw, automatic_randomization, augm_config)`: the reference's constructor, config keys,
    assertions, `randomize_augmentation()` and `augm_state`.  `draw(labels_seq)` resolves one sample's `SpatialAugmentState`
    with the reference's torch RNG calls in the reference's order, so after the same `torch.manual_seed` the draw equals the
    reference's, including its quirks: `th.randint(low=0, high=len - 1)` never picks the last label, the zoom-in factor is drawn
    at apply time, and a sequence without a non-empty label frame gets no zoom-in (with the reference's warning).
  * `sample_states(augmentor, labels_per_sample)`: one draw per sample of a batch, in batch order.
  * `augment_sequence(ev_seq, rows, count, states) -> (ev_out, rows_out, count_out, yolox)`: the batched form.
  * `augmentor(data_dict)`: the reference's call for ONE sequence (EV_REPR: list of T (C,H,W) uint8 device tensors,
    OBJLABELS_SEQ: list of T label tensors [n][7] or None).
  * `make_tables` / `write_tables` / `augment_planes` / `augment_labels`: the pieces, for callers that keep their buffers (nothing
    is allocated when `out` is given, so the two calls capture into a hipGraph and replay with a rewritten table).

Labels travel padded: rows fp32 [T][B][G][7] (t x y w h class_id class_confidence), count int32 [T][B] with -1 for a frame
without labels, which is also how a frame with zero labels must be passed (the reference's SparselyBatchedObjectLabels turns
an empty frame into None on construction; `pack_labels` does the same).  `labelled_frames(count_out, states)` gives the frames
the reference would still treat as labelled: count_out > 0, or count_out == 0 under zoom-out.  That is a reference quirk kept
visible: zoom-in sets a frame that lost every label to None, zoom-out keeps it as an empty label set.

Out of scope, each raises NotImplementedError naming the key: `rotate.prob > 0` (0 in every shipped config), vertical flip,
`DataType.FLOW` and `DataType.IMAGE`.  There is no PyTorch fallback: a missing kernel or an unsupported shape raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional, Sequence, Tuple, Union
from warnings import filterwarnings, warn

import numpy as np
import torch
import torch.distributions.categorical

from . import _lib as L
from .types import DataType

Tensor = torch.Tensor

NO_LABEL_WARN_MSG = 'No Labels found. This can lead to a crash and should not happen often.'
filterwarnings('always', message=NO_LABEL_WARN_MSG)

MODE_NONE, MODE_ZOOM_IN, MODE_ZOOM_OUT = 0, 1, 2
PLANES_TABLE_COLS, LABEL_TABLE_COLS = L.ENUMS['RVT_AUGMENT_PLANES_COLS'], L.ENUMS['RVT_AUGMENT_LABEL_COLS']


@dataclass
class ZoomOutState:
    active: bool
    x0: int
    y0: int
    zoom_out_factor: float


@dataclass
class RotationState:
    active: bool
    angle_deg: float


@dataclass
class AugmentationState:
    apply_h_flip: bool
    rotation: RotationState
    apply_zoom_in: bool
    zoom_out: ZoomOutState


@dataclass
class SpatialAugmentState:
    """One sample's resolved augmentation: what both kernels apply.  factor == 1 goes with mode 0."""
    flip: bool = False
    mode: int = MODE_NONE
    x0: int = 0
    y0: int = 0
    factor: float = 1.0

    def window_hw(self, hw: Tuple[int, int]) -> Tuple[int, int]:
        return int(hw[0] / self.factor), int(hw[1] / self.factor)


def _cfg(node: Any, key: str, *default):
    """node.key for attribute-style configs (DictConfig), node[key] for mappings; the default if the key is missing."""
    if isinstance(node, dict) or not hasattr(node, key):
        try:
            return node[key]
        except (KeyError, TypeError, IndexError):
            if default:
                return default[0]
            raise KeyError(key) from None
    return getattr(node, key)


def _has(node: Any, key: str) -> bool:
    try:
        return key in node
    except TypeError:
        return hasattr(node, key)


def torch_uniform_sample_scalar(min_value: float, max_value: float):
    """utils/helpers.py:6-10: no draw when the interval is a point."""
    assert max_value >= min_value, f'{max_value=} is smaller than {min_value=}'
    if max_value == min_value:
        return min_value
    return min_value + (max_value - min_value) * torch.rand(1).item()


def _label_array(lab) -> Optional[np.ndarray]:
    """A label frame as a CPU fp32 [n][7] array (None for a missing or empty frame)."""
    if lab is None:
        return None
    lab = getattr(lab, 'object_labels', lab)
    a = lab.detach().cpu().numpy() if torch.is_tensor(lab) else np.asarray(lab)
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 7)
    return a if a.shape[0] > 0 else None


def _sample_window_from_label(xywh, H, W, zh, zw) -> Tuple[int, int]:
    """randomly_sample_zoom_window_from_label_rectangle (augmentor.py:407-448), in Python double arithmetic."""
    assert H >= zh and W >= zw
    x0_l, y0_l, w_l, h_l = (float(v) for v in xywh)
    x1_l, y1_l = x0_l + w_l, y0_l + h_l
    assert x0_l >= 0 and y0_l >= 0 and w_l > 0 and h_l > 0
    assert x1_l <= W + 1e-2 - 1
    assert y1_l <= H + 1e-2 - 1
    x0_valid = max(x1_l - max(zw, w_l), 0)
    y0_valid = max(y1_l - max(zh, h_l), 0)
    x1_valid = min(x0_l + max(zw, w_l), W - 1)
    y1_valid = min(y0_l + max(zh, h_l), H - 1)
    x1_valid = max(x1_valid - zw, x0_valid)
    y1_valid = max(y1_valid - zh, y0_valid)
    x = int(torch_uniform_sample_scalar(min_value=x0_valid, max_value=x1_valid))
    assert 0 <= x < W
    y = int(torch_uniform_sample_scalar(min_value=y0_valid, max_value=y1_valid))
    assert 0 <= y < H
    return x, y


def _sample_window_from_objframe(frame: np.ndarray, H, W, zh, zw) -> Tuple[int, int]:
    """randomly_sample_zoom_window_from_objframe (augmentor.py:381-404): one candidate window per label (two draws each), then
    th.randint(low=0, high=len - 1), which never picks the last label."""
    samples = [_sample_window_from_label(frame[i, 1:5], H, W, zh, zw) for i in range(frame.shape[0])]
    assert len(samples) > 0
    idx = 0 if len(samples) == 1 else torch.randint(low=0, high=len(samples) - 1, size=(1,)).item()
    x0, y0 = samples[idx]
    assert W > x0 >= 0, f'{x0=}'
    assert H > y0 >= 0, f'{y0=}'
    return x0, y0


class RandomSpatialAugmentorGenX:
    def __init__(self, dataset_hw: Tuple[int, int], automatic_randomization: bool, augm_config: Any):
        assert isinstance(dataset_hw, tuple)
        assert len(dataset_hw) == 2
        assert all(x > 0 for x in dataset_hw)
        assert isinstance(automatic_randomization, bool)

        self.hw_tuple = dataset_hw
        self.automatic_randomization = automatic_randomization
        rotate, zoom = _cfg(augm_config, 'rotate'), _cfg(augm_config, 'zoom')
        self.h_flip_prob = _cfg(augm_config, 'prob_hflip')
        self.rot_prob = _cfg(rotate, 'prob')
        self.rot_min_angle_deg = _cfg(rotate, 'min_angle_deg', 0)
        self.rot_max_angle_deg = _cfg(rotate, 'max_angle_deg')
        self.zoom_prob = _cfg(zoom, 'prob')
        zoom_out = _cfg(zoom, 'zoom_out')
        zoom_out_weight = _cfg(zoom_out, 'weight', 1)
        self.min_zoom_out_factor = _cfg(_cfg(zoom_out, 'factor'), 'min')
        self.max_zoom_out_factor = _cfg(_cfg(zoom_out, 'factor'), 'max')
        has_zoom_in = _has(zoom, 'zoom_in')
        zoom_in = _cfg(zoom, 'zoom_in') if has_zoom_in else None
        zoom_in_weight = _cfg(zoom_in, 'weight') if has_zoom_in else 0
        self.min_zoom_in_factor = _cfg(_cfg(zoom_in, 'factor'), 'min') if has_zoom_in else 1
        self.max_zoom_in_factor = _cfg(_cfg(zoom_in, 'factor'), 'max') if has_zoom_in else 1

        assert 0 <= self.h_flip_prob <= 1
        assert 0 <= self.rot_prob <= 1
        assert 0 <= self.rot_min_angle_deg <= self.rot_max_angle_deg
        assert 0 <= self.zoom_prob <= 1
        assert 0 <= zoom_in_weight
        assert self.max_zoom_in_factor >= self.min_zoom_in_factor >= 1
        assert 0 <= zoom_out_weight
        assert self.max_zoom_out_factor >= self.min_zoom_out_factor >= 1
        if not automatic_randomization:
            # streaming datasets: zoom-in depends on the labels and cannot be drawn ahead of the data
            assert zoom_in_weight == 0, f'{zoom_in_weight=}'
        if self.rot_prob > 0:
            raise NotImplementedError('rotate.prob > 0: rotation is not implemented on the device (0 in every shipped config)')
        if _cfg(augm_config, 'prob_vflip', 0):
            raise NotImplementedError('prob_vflip: vertical flip is not implemented (the reference has no config key for it either)')

        self.zoom_in_or_out_distribution = torch.distributions.categorical.Categorical(
            probs=torch.tensor([zoom_in_weight, zoom_out_weight]))

        self.augm_state = AugmentationState(
            apply_h_flip=False,
            rotation=RotationState(active=False, angle_deg=0.0),
            apply_zoom_in=False,
            zoom_out=ZoomOutState(active=False, x0=0, y0=0, zoom_out_factor=1.0))

    def randomize_augmentation(self):
        """The input-independent part of the draw (augmentor.py:89-121), same torch RNG calls in the same order."""
        self.augm_state.apply_h_flip = self.h_flip_prob > torch.rand(1).item()

        self.augm_state.rotation.active = self.rot_prob > torch.rand(1).item()       # rot_prob == 0: never active, the draw stays
        assert not self.augm_state.rotation.active

        do_zoom = self.zoom_prob > torch.rand(1).item()
        do_zoom_in = self.zoom_in_or_out_distribution.sample().item() == 0
        do_zoom_out = not do_zoom_in
        do_zoom_in &= do_zoom
        do_zoom_out &= do_zoom
        self.augm_state.apply_zoom_in = do_zoom_in
        self.augm_state.zoom_out.active = do_zoom_out
        if do_zoom_out:
            rand_zoom_out_factor = torch_uniform_sample_scalar(
                min_value=self.min_zoom_out_factor, max_value=self.max_zoom_out_factor)
            height, width = self.hw_tuple
            zoom_window_h, zoom_window_w = int(height / rand_zoom_out_factor), int(width / rand_zoom_out_factor)
            x0_sampled = int(torch_uniform_sample_scalar(min_value=0, max_value=width - zoom_window_w))
            y0_sampled = int(torch_uniform_sample_scalar(min_value=0, max_value=height - zoom_window_h))
            self.augm_state.zoom_out.x0 = x0_sampled
            self.augm_state.zoom_out.y0 = y0_sampled
            self.augm_state.zoom_out.zoom_out_factor = rand_zoom_out_factor

    def draw(self, labels_seq: Sequence[Any]) -> SpatialAugmentState:
        """One sample's state: randomize_augmentation() (if automatic), then what the reference's __call__ draws while it
        applies the state.  labels_seq: the sample's T label frames on the CPU ([n][7] tensors / arrays, None where missing);
        only zoom-in reads them: the window is sampled around the labels of the most recent non-empty frame AFTER the flip."""
        if self.automatic_randomization:
            self.randomize_augmentation()
        st = self.augm_state
        H, W = self.hw_tuple
        out = SpatialAugmentState(flip=bool(st.apply_h_flip))
        if st.apply_zoom_in:
            f = torch_uniform_sample_scalar(min_value=self.min_zoom_in_factor, max_value=self.max_zoom_in_factor)
            if f == 1:
                return out
            zh, zw = int(H / f), int(W / f)
            latest = None
            for lab in reversed(list(labels_seq)):
                latest = _label_array(lab)
                if latest is not None:
                    break
            if latest is None:
                warn(message=NO_LABEL_WARN_MSG, category=UserWarning, stacklevel=2)
                return out
            if out.flip:                                  # flip_lr_ on the fp32 rows: (W-1 - x) - w, two rounded operations
                latest = latest.copy()
                latest[:, 1] = (np.float32(W - 1) - latest[:, 1]) - latest[:, 3]
            out.x0, out.y0 = _sample_window_from_objframe(latest, H, W, zh, zw)
            out.mode, out.factor = MODE_ZOOM_IN, float(f)
        if st.zoom_out.active:
            assert not st.apply_zoom_in
            if st.zoom_out.zoom_out_factor != 1:
                out.mode, out.factor = MODE_ZOOM_OUT, float(st.zoom_out.zoom_out_factor)
                out.x0, out.y0 = int(st.zoom_out.x0), int(st.zoom_out.y0)
        return out

    def augment_sequence(self, ev_seq, rows: Tensor, count: Tensor, states: Sequence[SpatialAugmentState]):
        return augment_sequence(ev_seq, rows, count, states, self.hw_tuple)

    def __call__(self, data_dict):
        """The reference's call for one sequence.  Values under EV_REPR (list of T (C,H,W) uint8 device tensors) and
        OBJLABELS_SEQ (list of T [n][7] tensors or None) are replaced; the masks pass through."""
        for k in data_dict:
            if k in (DataType.FLOW, DataType.IMAGE):
                raise NotImplementedError(f'{k}: only DataType.EV_REPR planes and object labels are augmented on the device')
        ev = list(data_dict[DataType.EV_REPR])
        labels = list(data_dict[DataType.OBJLABELS_SEQ])
        assert len(ev) == len(labels) and tuple(ev[0].shape[-2:]) == tuple(self.hw_tuple)
        state = self.draw(labels)
        dev = ev[0].device
        rows, count = pack_labels([[lab] for lab in labels], device=dev)
        ev_out, rows_out, count_out, _ = augment_sequence([e.unsqueeze(0) for e in ev], rows, count, [state], self.hw_tuple)
        keep = labelled_frames(count_out, [state]).cpu()
        counts = count_out.cpu()
        out = dict(data_dict)
        out[DataType.EV_REPR] = [ev_out[t, 0] for t in range(len(ev))]
        out[DataType.OBJLABELS_SEQ] = [rows_out[t, 0, :max(int(counts[t, 0]), 0)].clone() if bool(keep[t, 0]) else None
                                       for t in range(len(ev))]
        return out


def sample_states(augmentor: RandomSpatialAugmentorGenX, labels_per_sample: Sequence[Sequence[Any]]) -> List[SpatialAugmentState]:
    """One draw per sample, in batch order.  labels_per_sample[b]: sample b's T label frames (CPU copies)."""
    return [augmentor.draw(seq) for seq in labels_per_sample]


def pack_labels(labels_seq: Sequence[Sequence[Any]], G: Optional[int] = None, device=None) -> Tuple[Tensor, Tensor]:
    """labels_seq[t][b] ([n][7] or None) -> rows fp32 [T][B][G][7], count int32 [T][B]; empty and missing frames get -1."""
    T, B = len(labels_seq), len(labels_seq[0])
    arrs = [[_label_array(lab) for lab in frame] for frame in labels_seq]
    n_max = max([a.shape[0] for frame in arrs for a in frame if a is not None], default=0)
    G = max(n_max, 1) if G is None else int(G)
    assert G >= max(n_max, 1), f'G={G} smaller than the largest frame ({n_max} labels)'
    rows = np.zeros((T, B, G, 7), dtype=np.float32)
    count = np.full((T, B), -1, dtype=np.int32)
    for t in range(T):
        for b in range(B):
            a = arrs[t][b]
            if a is not None:
                rows[t, b, :a.shape[0]] = a
                count[t, b] = a.shape[0]
    rows, count = torch.from_numpy(rows), torch.from_numpy(count)
    return (rows, count) if device is None else (rows.to(device), count.to(device))


def _check_state(s: SpatialAugmentState, H: int, W: int) -> None:
    if s.mode not in (MODE_NONE, MODE_ZOOM_IN, MODE_ZOOM_OUT):
        raise ValueError(f'mode {s.mode} is not 0 (none), 1 (zoom-in) or 2 (zoom-out)')
    if s.mode == MODE_NONE:
        return
    if not s.factor > 1:
        raise ValueError(f'zoom factor {s.factor} must be > 1 (a factor of exactly 1 is mode 0)')
    zh, zw = s.window_hw((H, W))
    if zh < 1 or zw < 1 or s.x0 < 0 or s.y0 < 0 or s.x0 + zw > W or s.y0 + zh > H:
        raise ValueError(f'zoom window x0={s.x0} y0={s.y0} {zh}x{zw} lies outside the {H}x{W} frame')


def host_tables(states: Sequence[SpatialAugmentState], hw: Tuple[int, int]) -> Tuple[np.ndarray, np.ndarray]:
    """The two per-sample tables (include/rvt_hip.h): int32 [B][8] for the planes, fp32 [B][12] for the labels.  Every fp32
    constant is computed in Python double arithmetic as the reference does and rounded once."""
    H, W = hw
    it = np.zeros((len(states), PLANES_TABLE_COLS), dtype=np.int32)
    ft = np.zeros((len(states), LABEL_TABLE_COLS), dtype=np.float64)
    for b, s in enumerate(states):
        _check_state(s, H, W)
        zh, zw = s.window_hw(hw) if s.mode != MODE_NONE else (H, W)
        it[b, :6] = (int(s.flip), s.mode, s.x0, s.y0, zh, zw)
        ft[b, :5] = (float(s.flip), s.mode, W - 1, s.x0, s.y0)
        f = s.factor
        if s.mode == MODE_ZOOM_IN:
            zh_f, zw_f = H / f, W / f                                  # NOT truncated (labels.py:271)
            ft[b, 5:10] = (min(s.x0 + zw_f, W - 1) - 1, min(s.y0 + zh_f, H - 1) - 1, f, f * zw_f - 1, f * zh_f - 1)
        elif s.mode == MODE_ZOOM_OUT:
            m = 1 / f
            ft[b, 5:10] = (0, 0, m, m * W - 1, m * H - 1)
    return it, ft.astype(np.float32)


def make_tables(states: Sequence[SpatialAugmentState], hw: Tuple[int, int], device) -> Tuple[Tensor, Tensor]:
    it, ft = host_tables(states, hw)
    return torch.from_numpy(it).to(device), torch.from_numpy(ft).to(device)


def write_tables(states: Sequence[SpatialAugmentState], hw: Tuple[int, int], planes_table: Tensor, label_table: Tensor) -> None:
    """Rewrite existing device tables in place (same addresses: a captured graph replays with the new parameters)."""
    it, ft = host_tables(states, hw)
    assert tuple(planes_table.shape) == it.shape and tuple(label_table.shape) == ft.shape
    planes_table.copy_(torch.from_numpy(it))
    label_table.copy_(torch.from_numpy(ft))


def _check_u8(t: Tensor, what: str) -> None:
    if t.dtype != torch.uint8:
        raise TypeError(f'{what} must be uint8 event planes, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{what} must be contiguous')


def augment_planes(ev_seq: Union[Tensor, Sequence[Tensor]], planes_table: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """ev_seq: (T,B,C,H,W) uint8, or a list of T separately allocated (B,C,H,W) tensors (one launch each, no stacking copy).
    Returns out (T,B,C,H,W), allocated unless given; it must not share memory with the input."""
    B = planes_table.shape[0]
    if planes_table.dtype != torch.int32 or planes_table.dim() != 2 or planes_table.shape[1] != PLANES_TABLE_COLS:
        raise ValueError(f'planes_table must be int32 [B][{PLANES_TABLE_COLS}]')
    if torch.is_tensor(ev_seq):
        if ev_seq.dim() != 5 or ev_seq.shape[1] != B:
            raise ValueError(f'ev_seq must be (T, B={B}, C, H, W), got {tuple(ev_seq.shape)}')
        _check_u8(ev_seq, 'ev_seq')
        srcs, shape = [ev_seq], tuple(ev_seq.shape)
    else:
        srcs = list(ev_seq)
        for t, e in enumerate(srcs):
            if e.dim() != 4 or e.shape != srcs[0].shape or e.shape[0] != B:
                raise ValueError(f'ev_seq[{t}] must be (B={B}, C, H, W) like ev_seq[0], got {tuple(e.shape)}')
            _check_u8(e, f'ev_seq[{t}]')
        shape = (len(srcs),) + tuple(srcs[0].shape)
    dev = srcs[0].device
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
        raise ValueError(f'out must be contiguous uint8 {shape} on {dev}')
    _, _, C, H, W = shape
    st = L.stream_of(out)
    if len(srcs) == 1 and srcs[0].dim() == 5:
        L.call('rvt_augment_planes', L.ptr(srcs[0]), L.ptr(out), L.ptr(planes_table), shape[0] * B, B, C, H, W, st)
    else:
        for t, e in enumerate(srcs):
            L.call('rvt_augment_planes', L.ptr(e), L.ptr(out[t]), L.ptr(planes_table), B, B, C, H, W, st)
    return out


def augment_labels(rows: Tensor, count: Tensor, label_table: Tensor, out: Optional[Tuple[Tensor, Tensor, Optional[Tensor]]] = None,
                   yolox: bool = True) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """rows fp32 [T][B][G][7], count int32 [T][B] -> (rows_out, count_out, yolox [T][B][G][5] or None)."""
    B = label_table.shape[0]
    if label_table.dtype != torch.float32 or label_table.dim() != 2 or label_table.shape[1] != LABEL_TABLE_COLS:
        raise ValueError(f'label_table must be float32 [B][{LABEL_TABLE_COLS}]')
    if rows.dtype != torch.float32 or rows.dim() != 4 or rows.shape[1] != B or rows.shape[3] != 7:
        raise TypeError(f'rows must be float32 [T][B={B}][G][7], got {rows.dtype} {tuple(rows.shape)}')
    T, _, G, _ = rows.shape
    if count.dtype != torch.int32 or tuple(count.shape) != (T, B):
        raise TypeError(f'count must be int32 [T={T}][B={B}], got {count.dtype} {tuple(count.shape)}')
    if G < 1:
        raise ValueError('rows needs room for at least one label per frame (G >= 1)')
    if out is None:
        out = (torch.empty_like(rows), torch.empty_like(count),
               torch.empty(T, B, G, 5, dtype=torch.float32, device=rows.device) if yolox else None)
    rows_out, count_out, yo = out
    for t, ref, cols in ((rows_out, rows, 7), (count_out, count, None), (yo, rows, 5)):
        if t is None:
            continue
        shp = tuple(ref.shape) if cols in (7, None) else (T, B, G, 5)
        if tuple(t.shape) != shp or t.dtype != ref.dtype or t.device != rows.device or not t.is_contiguous():
            raise ValueError(f'out tensor must be contiguous {ref.dtype} {shp} on {rows.device}')
    L.call('rvt_augment_labels', L.ptr(rows), L.ptr(count), L.ptr(label_table), T * B, B, G, L.ptr(rows_out), L.ptr(count_out),
           L.ptr(yo), L.stream_of(rows))
    return rows_out, count_out, yo


def augment_sequence(ev_seq, rows: Tensor, count: Tensor, states: Sequence[SpatialAugmentState],
                     hw: Optional[Tuple[int, int]] = None):
    """Flip / zoom a batch of sequences and their labels: (ev_out (T,B,C,H,W), rows_out, count_out, yolox [T][B][G][5])."""
    first = ev_seq if torch.is_tensor(ev_seq) else ev_seq[0]
    frame_hw = (int(first.shape[-2]), int(first.shape[-1]))
    if hw is not None and tuple(hw) != frame_hw:
        raise ValueError(f'event planes are {frame_hw}, the augmentor was built for {tuple(hw)}')
    it, ft = make_tables(states, frame_hw, first.device)
    ev_out = augment_planes(ev_seq, it)
    rows_out, count_out, yolox = augment_labels(rows, count, ft)
    return ev_out, rows_out, count_out, yolox


def labelled_frames(count_out: Tensor, states: Sequence[SpatialAugmentState]) -> Tensor:
    """bool [T][B]: the frames the reference still treats as labelled after the augmentation (see the module docstring)."""
    zoom_out = torch.tensor([s.mode == MODE_ZOOM_OUT for s in states], dtype=torch.bool, device=count_out.device)
    return (count_out > 0) | ((count_out == 0) & zoom_out.unsqueeze(0))
