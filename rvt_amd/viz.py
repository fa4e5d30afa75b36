"""Detection previews on the device: event planes and box lists to RGB images in one launch (csrc/capi_viz.hip: rvt_render_preview).

Mirror of the reference's detection visualisation callback: `VizCallbackBase.ev_repr_to_img` (callbacks/viz_base.py:164-174) turns an
event tensor into a grey / white / black image, `DetectionVizCallback` (callbacks/detection.py:36-69) draws the predicted and the
labelled boxes into one copy each and stacks the prediction image above the label image.  The reference copies every tensor to the
host first; here planes, detections and labels stay where the loader and the post-processing left them and nothing synchronises with
the host.  include/rvt_hip.h states the rendering rule; it is integer work and bit-exact.

  * `render_preview(planes, det, det_count, label_rows, label_count, frame_index, ...)` -> uint8 [Fout][P*Hs][Ws][3].
  * `ev_repr_to_img(planes)`: one panel, no boxes.
  * `DetectionPreview(dataset, n_samples, every_n_steps)`: the callback's frame choice on the loader's batch; keeps the rendered
    device tensors, `save(path)` writes them as binary PPM (and PNG when PIL is there).

Not restated: cv2's HSV colour map and Hershey font (`draw_bboxes`), bbox_visualizer's INTER_AREA resize, wandb logging, the
grad-flow figure.  The class colours and the short label maps are the reference's fixed ones (vis_utils.py:11-13, 49-60); the 5 x 7
glyphs are this package's own.  There is no PyTorch fallback: a missing kernel or an unsupported shape raises.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from .types import DataType

Tensor = torch.Tensor

KIND_DET, KIND_LABEL = L.ENUMS['RVT_VIZ_KIND_DET'], L.ENUMS['RVT_VIZ_KIND_LABEL']
FLAG_TEXT = L.ENUMS['RVT_VIZ_TEXT']
STATUS_INDEX = L.ENUMS['RVT_VIZ_STATUS_INDEX']
MAX_BOXES, NAME_BYTES, GLYPH_ROWS = L.ENUMS['RVT_VIZ_MAX_BOXES'], L.ENUMS['RVT_VIZ_NAME_BYTES'], L.ENUMS['RVT_VIZ_GLYPH_ROWS']
SCALES = (1, 2, 4)

# vis_utils.py:11-13 and 49-60: the short label maps and the fixed class colours (rgb)
LABELMAPS = {'gen1': ('car', 'pedestrian'), 'gen4': ('pedestrian', 'two wheeler', 'car')}
PALETTES = {'gen1': ((255, 255, 0), (0, 0, 255)), 'gen4': ((0, 0, 255), (0, 255, 255), (255, 255, 0))}

# 5 x 7 glyphs, one hex byte per row from the top, bit 4 the leftmost pixel.  A character that is not listed draws nothing.
_GLYPHS = {
    '0': '0e11131519110e', '1': '040c040404040e', '2': '0e11010204081f', '3': '1f02040201110e', '4': '02060a121f0202',
    '5': '1f101e0101110e', '6': '0608101e11110e', '7': '1f010204080808', '8': '0e11110e11110e', '9': '0e11110f01020c',
    '.': '00000000000c0c', '-': '0000001f000000', '_': '0000000000001f', ':': '000c0c000c0c00', '/': '00010204081000',
    '?': '0e110102040004', '%': '18190204081303', '+': '0004041f040400',
    'a': '00000e010f110f', 'b': '1010161911111e', 'c': '00000e1010110e', 'd': '01010d1311110f',
    'e': '00000e111f100e', 'f': '0609081c080808', 'g': '000f11110f010e', 'h': '10101619111111', 'i': '04000c0404040e',
    'j': '0200060202120c', 'k': '10101214181412', 'l': '0c04040404040e', 'm': '00001a15151111', 'n': '00001619111111',
    'o': '00000e1111110e', 'p': '00001e111e1010', 'q': '00000d130f0101', 'r': '00001619101010', 's': '00000e100e011e',
    't': '08081c08080906', 'u': '0000111111130d', 'v': '00001111110a04', 'w': '0000111115150a', 'x': '0000110a040a11',
    'y': '000011110f010e', 'z': '00001f0204081f',
    'A': '0e1111111f1111', 'B': '1e11111e11111e', 'C': '0e11101010110e', 'D': '1c12111111121c', 'E': '1f10101e10101f',
    'F': '1f10101e101010', 'G': '0e11101711110f', 'H': '1111111f111111', 'I': '0e04040404040e', 'J': '0702020202120c',
    'K': '11121418141211', 'L': '1010101010101f', 'M': '111b1515111111', 'N': '11111915131111', 'O': '0e11111111110e',
    'P': '1e11111e101010', 'Q': '0e11111115120d', 'R': '1e11111e141211', 'S': '0f10100e01011e', 'T': '1f040404040404',
    'U': '1111111111110e', 'V': '11111111110a04', 'W': '1111111515150a', 'X': '11110a040a1111', 'Y': '1111110a040404',
    'Z': '1f01020408101f',
}


def glyph_table() -> np.ndarray:
    """uint8 [128][7]: the row bitmaps of every ASCII character (zero rows: the character draws nothing)."""
    g = np.zeros((128, GLYPH_ROWS), dtype=np.uint8)
    for ch, rows in _GLYPHS.items():
        g[ord(ch)] = np.frombuffer(bytes.fromhex(rows), dtype=np.uint8)
    return g


def name_table(names: Sequence[str]) -> np.ndarray:
    """uint8 [n][12]: zero-terminated ASCII, a longer name cut to 12 characters."""
    if len(names) < 1:
        raise ValueError('names must hold at least one class name')
    t = np.zeros((len(names), NAME_BYTES), dtype=np.uint8)
    for i, n in enumerate(names):
        b = str(n).encode('ascii')[:NAME_BYTES]
        if 0 in b:
            raise ValueError(f'class name {n!r} holds a zero byte')
        t[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return t


_TABLES: Dict[Tuple, Tuple[Tensor, Tensor]] = {}
_GLYPH_DEV: Dict[Tuple, Tensor] = {}
_STATUS: Dict[Tuple, Tensor] = {}


def _dev_key(device) -> Tuple:
    device = torch.device(device)
    return device.type, device.index


def default_tables(dataset: str, device) -> Tuple[Tensor, Tensor]:
    """(palette uint8 [n][3], names uint8 [n][12]) of a dataset on a device, built once per device."""
    if dataset not in LABELMAPS:
        raise ValueError(f'dataset must be one of {sorted(LABELMAPS)}, got {dataset!r}')
    key = (dataset,) + _dev_key(device)
    if key not in _TABLES:
        _TABLES[key] = (torch.tensor(PALETTES[dataset], dtype=torch.uint8).to(device),
                        torch.from_numpy(name_table(LABELMAPS[dataset])).to(device))
    return _TABLES[key]


def glyphs_on(device) -> Tensor:
    key = _dev_key(device)
    if key not in _GLYPH_DEV:
        _GLYPH_DEV[key] = torch.from_numpy(glyph_table()).to(device)
    return _GLYPH_DEV[key]


def _table(t, cols: int, what: str, device) -> Tensor:
    if not torch.is_tensor(t):
        t = torch.from_numpy(name_table(t)) if what == 'names' else torch.tensor(t, dtype=torch.uint8)
        t = t.to(device)
    if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != cols or t.shape[0] < 1:
        raise TypeError(f'{what} must be uint8 [n][{cols}], got {t.dtype} {tuple(t.shape)}')
    if t.device != device or not t.is_contiguous():
        raise ValueError(f'{what} must be contiguous on {device}')
    return t


def _boxes(rows: Optional[Tensor], count: Optional[Tensor], lead: Tuple[int, ...], device, what: str):
    """A panel's (rows fp32 [F][N][7], count int32 [F], N) from rows shaped lead + (N, 7) and count shaped lead; (None, None, 0)."""
    if rows is None:
        if count is not None:
            raise ValueError(f'{what}_count without {what} rows')
        return None, None, 0
    if count is None:
        raise ValueError(f'{what} rows without {what}_count')
    if rows.dtype != torch.float32 or rows.dim() != len(lead) + 2 or tuple(rows.shape[:-2]) != lead or rows.shape[-1] != 7:
        raise TypeError(f'{what} rows must be float32 {list(lead)}[N][7], got {rows.dtype} {tuple(rows.shape)}')
    if count.dtype != torch.int32 or tuple(count.shape) != lead:
        raise TypeError(f'{what} count must be int32 {list(lead)}, got {count.dtype} {tuple(count.shape)}')
    if rows.shape[-2] < 1:
        raise ValueError(f'{what} rows need room for at least one box per frame (N >= 1)')
    for t, n in ((rows, 'rows'), (count, 'count')):
        if t.device != device or not t.is_contiguous():
            raise ValueError(f'{what} {n} must be contiguous on {device}')
    return rows, count, int(rows.shape[-2])


def render_preview(planes: Tensor, det: Optional[Tensor] = None, det_count: Optional[Tensor] = None, label_rows: Optional[Tensor] = None,
                   label_count: Optional[Tensor] = None, frame_index: Optional[Tensor] = None, dataset: str = 'gen1', palette=None,
                   names=None, scale: int = 1, text: bool = True, out: Optional[Tensor] = None, status: Optional[Tensor] = None) -> Tensor:
    """planes (F,C,H,W) or (T,B,C,H,W), uint8 or int8; det fp32 [F][max_det][7] with det_count int32 [F] as `postprocess_padded`
    returns them, label_rows fp32 [F][G][7] with label_count int32 [F] as `augment.pack_labels` lays them out (both with the planes'
    leading dimensions).  Returns uint8 [Fout][P*Hs][Ws][3]: one panel per box list given, predictions above labels; one panel without
    boxes when none is given.  frame_index int64 [Fout] on the device picks and orders the frames (-1: a black image), None renders
    all F.  palette uint8 [n][3] / names (strings, or uint8 [n][12]) replace the dataset's defaults.  Nothing is allocated when `out`
    (and, for a caller that reads it, `status` int32 [1], or-ed with 1 by a frame index outside [-1, F)) is given."""
    if not torch.is_tensor(planes) or planes.dtype not in (torch.uint8, torch.int8):
        raise TypeError(f'planes must be uint8 or int8 event planes, got {getattr(planes, "dtype", type(planes))}')
    if planes.dim() not in (4, 5):
        raise ValueError(f'planes must be (F, C, H, W) or (T, B, C, H, W), got {tuple(planes.shape)}')
    if not planes.is_contiguous():
        raise ValueError('planes must be contiguous')
    lead = tuple(planes.shape[:-3])
    C, H, W = (int(v) for v in planes.shape[-3:])
    F = int(np.prod(lead))
    if C < 2 or C % 2:
        raise ValueError(f'planes need an even number of channels >= 2 (negative half, positive half), got C={C}')
    if F < 1 or H < 1 or W < 1:
        raise ValueError(f'planes {tuple(planes.shape)} hold no pixel')
    if scale not in SCALES:
        raise ValueError(f'scale must be one of {SCALES}, got {scale}')
    dev = planes.device
    panels = [(r, c, n, k) for r, c, n, k in (_boxes(det, det_count, lead, dev, 'det') + (KIND_DET,),
                                              _boxes(label_rows, label_count, lead, dev, 'label') + (KIND_LABEL,)) if r is not None]
    P = max(len(panels), 1)
    panels += [(None, None, 0, 0)] * (2 - len(panels))
    if frame_index is None:
        Fout = F
    else:
        if frame_index.dtype != torch.int64 or frame_index.dim() != 1 or frame_index.shape[0] < 1:
            raise TypeError(f'frame_index must be int64 [Fout], got {frame_index.dtype} {tuple(frame_index.shape)}')
        if frame_index.device != dev or not frame_index.is_contiguous():
            raise ValueError(f'frame_index must be contiguous on {dev}')
        Fout = int(frame_index.shape[0])
    d_pal, d_names = (None, None) if palette is not None and names is not None else default_tables(dataset, dev)
    pal = d_pal if palette is None else _table(palette, 3, 'palette', dev)
    nam = d_names if names is None else _table(names, NAME_BYTES, 'names', dev)
    shape = (Fout, P * H * scale, W * scale, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
        raise ValueError(f'out must be contiguous uint8 {shape} on {dev}')
    if status is None:
        status = _STATUS.get(_dev_key(dev))
        if status is None:
            status = _STATUS[_dev_key(dev)] = torch.zeros(1, dtype=torch.int32, device=dev)
    elif status.dtype != torch.int32 or status.numel() != 1 or status.device != dev:
        raise ValueError(f'status must be int32 [1] on {dev}')
    (r0, c0, n0, k0), (r1, c1, n1, k1) = panels
    L.call('rvt_render_preview', L.ptr(planes), int(planes.dtype == torch.int8), F, C, H, W, L.ptr(r0), L.ptr(c0), n0, k0, L.ptr(r1),
           L.ptr(c1), n1, k1, P, L.ptr(frame_index), Fout, L.ptr(pal), int(pal.shape[0]), L.ptr(nam), int(nam.shape[0]),
           L.ptr(glyphs_on(dev)), int(scale), FLAG_TEXT if text else 0, L.ptr(out), L.ptr(status), L.stream_of(out))
    return out


def ev_repr_to_img(planes: Tensor) -> Tensor:
    """The reference's `ev_repr_to_img` for every frame: uint8 [F][H][W][3], grey where the two halves of the channels cancel,
    white where the second half outweighs the first, black where the first outweighs the second."""
    return render_preview(planes, text=False)


def last_labelled(labelled: Tensor, n_samples: int) -> Tensor:
    """int64 [n_samples]: the flat (t * B + b) indices of the last n_samples labelled frames, the last one first, -1 where the
    batch has fewer (callbacks/detection.py:48-51 on the step's list of labelled frames).  No host synchronisation."""
    flat = labelled.reshape(-1)
    n = min(int(n_samples), flat.numel())
    pos = torch.arange(flat.numel(), dtype=torch.int64, device=flat.device)
    idx = torch.topk(torch.where(flat.bool(), pos, torch.full_like(pos, -1)), n).values
    return idx.contiguous()


def write_ppm(img: Union[Tensor, np.ndarray], path: str) -> None:
    """One uint8 [H][W][3] image as binary PPM (P6)."""
    a = img.detach().cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise TypeError(f'an image is uint8 [H][W][3], got {a.dtype} {a.shape}')
    with open(path, 'wb') as f:
        f.write(b'P6\n%d %d\n255\n' % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a).tobytes())


class DetectionPreview:
    """The reference's training-time detection preview on the loader's batch: every `every_n_steps` steps the last `n_samples`
    labelled frames of the batch, predictions above labels.  Only the frame choice and the rendering of Lightning's callback are
    restated; logging is the caller's (`images()`, `save()`)."""

    def __init__(self, dataset: str = 'gen1', n_samples: int = 8, every_n_steps: int = 500, scale: int = 1, text: bool = True, keep: int = 4):
        if dataset not in LABELMAPS:
            raise ValueError(f'dataset must be one of {sorted(LABELMAPS)}, got {dataset!r}')
        if n_samples < 1 or every_n_steps < 1 or keep < 1:
            raise ValueError('n_samples, every_n_steps and keep must be positive')
        self.dataset, self.n_samples, self.every_n_steps, self.scale, self.text, self.keep = dataset, n_samples, every_n_steps, scale, text, keep
        self._kept: List[Tuple[int, Tensor]] = []

    def on_train_batch(self, step: int, batch: dict, det: Optional[Tensor] = None, det_count: Optional[Tensor] = None) -> Optional[Tensor]:
        """batch: one batch of `BatchLoader`; det [T][B][max_det][7] / det_count [T][B]: the step's detections of every frame (None:
        the label panel alone).  Returns the rendered uint8 [n][P*Hs][Ws][3] device tensor, None on a step that is not due."""
        if step % self.every_n_steps:
            return None
        ev = batch['data'][DataType.EV_REPR]
        if not torch.is_tensor(ev):
            ev = torch.stack(list(ev))                          # (a MIXED part batch carries a list over t)
        rows, count, _, labelled = batch['device_labels']
        index = last_labelled(labelled, self.n_samples)
        img = render_preview(ev, det, det_count, rows, count, frame_index=index, dataset=self.dataset, scale=self.scale, text=self.text)
        self._kept.append((int(step), img))
        del self._kept[:-self.keep]
        return img

    def images(self) -> List[Tuple[int, Tensor]]:
        """(step, uint8 [n][P*Hs][Ws][3] device tensor) of the kept renderings, oldest first."""
        return list(self._kept)

    def save(self, path: str) -> List[str]:
        """Every kept image as `<path>/step<step>_<i>.ppm`, and as .png beside it when PIL imports.  Returns the files written."""
        try:
            from PIL import Image
        except ImportError:
            Image = None
        os.makedirs(path, exist_ok=True)
        written = []
        for step, imgs in self._kept:
            host = imgs.cpu().numpy()
            for i in range(host.shape[0]):
                stem = os.path.join(path, f'step{step:08d}_{i}')
                write_ppm(host[i], stem + '.ppm')
                written.append(stem + '.ppm')
                if Image is not None:
                    Image.fromarray(host[i]).save(stem + '.png')
                    written.append(stem + '.png')
        return written
