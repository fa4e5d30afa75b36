"""Plain-torch restatement of the reference's spatial augmentation of one resolved state (data/utils/augmentor.py tensor
branches, data/genx_utils/labels.py label transforms): th.flip, interpolate(mode='nearest-exact') on a crop / into a zero canvas,
and the per-frame label arithmetic with Python scalars on fp32 tensors.  TEST INFRASTRUCTURE: pinned to the reference fixtures by
tests/test_augment.py::test_restatement_matches_reference_golden, and the "what a user had before" baseline of
profiles/bench_augment.py.  States are rvt_amd.augment.SpatialAugmentState-like objects (flip, mode, x0, y0, factor)."""
import torch
from torch.nn.functional import interpolate


def planes_ref(ev: torch.Tensor, states) -> torch.Tensor:
    """ev (T,B,C,H,W) uint8 -> augmented (T,B,C,H,W), sample by sample as the reference does."""
    T, B, C, H, W = ev.shape
    out = torch.empty_like(ev)
    for b, s in enumerate(states):
        x = ev[:, b]
        if s.flip:
            x = torch.flip(x, dims=[-1])
        if s.mode == 1 and s.factor != 1:
            zh, zw = int(H / s.factor), int(W / s.factor)
            x = interpolate(x[..., s.y0:s.y0 + zh, s.x0:s.x0 + zw], size=(H, W), mode='nearest-exact')
        elif s.mode == 2 and s.factor != 1:
            zh, zw = int(H / s.factor), int(W / s.factor)
            win = interpolate(x, size=(zh, zw), mode='nearest-exact')
            x = torch.zeros_like(x)
            x[..., s.y0:s.y0 + zh, s.x0:s.x0 + zw] = win
        out[:, b] = x
    return out


def _scale(lab: torch.Tensor, m: float, hw):
    """ObjectLabels.scale_: returns (rows, new input_size_hw)."""
    if lab.shape[0] == 0 or m == 1:
        return lab, hw
    new_h, new_w = m * hw[0], m * hw[1]
    x1 = torch.clamp((lab[:, 1] + lab[:, 3]) * m, max=new_w - 1)
    y1 = torch.clamp((lab[:, 2] + lab[:, 4]) * m, max=new_h - 1)
    lab[:, 1] = lab[:, 1] * m
    lab[:, 2] = lab[:, 2] * m
    lab[:, 3] = x1 - lab[:, 1]
    lab[:, 4] = y1 - lab[:, 2]
    return lab[(lab[:, 3] > 0) & (lab[:, 4] > 0)], (new_h, new_w)


def labels_frame_ref(lab: torch.Tensor, s, hw) -> torch.Tensor:
    """One non-empty frame [n][7] -> its surviving rows [k][7] (k may be 0)."""
    H, W = hw
    lab = lab.clone()
    if s.flip:
        lab[:, 1] = W - 1 - lab[:, 1] - lab[:, 3]
    if s.mode == 1 and s.factor != 1:
        f = s.factor
        zh_f, zw_f = H / f, W / f
        z_x1, z_y1 = min(s.x0 + zw_f, W - 1), min(s.y0 + zh_f, H - 1)
        x0 = torch.clamp(lab[:, 1], min=s.x0, max=z_x1 - 1)
        y0 = torch.clamp(lab[:, 2], min=s.y0, max=z_y1 - 1)
        x1 = torch.clamp(lab[:, 1] + lab[:, 3], min=s.x0, max=z_x1 - 1)
        y1 = torch.clamp(lab[:, 2] + lab[:, 4], min=s.y0, max=z_y1 - 1)
        lab[:, 1] = x0 - s.x0
        lab[:, 2] = y0 - s.y0
        lab[:, 3] = x1 - x0
        lab[:, 4] = y1 - y0
        lab = lab[(lab[:, 3] > 0) & (lab[:, 4] > 0)]
        lab, _ = _scale(lab, f, (zh_f, zw_f))
    elif s.mode == 2 and s.factor != 1:
        lab, _ = _scale(lab, 1 / s.factor, (H, W))
        if lab.shape[0] > 0:
            lab[:, 1] = lab[:, 1] + s.x0
            lab[:, 2] = lab[:, 2] + s.y0
    return lab


def labels_ref(rows: torch.Tensor, count: torch.Tensor, states, hw):
    """Padded form: rows [T][B][G][7], count [T][B] -> (rows_out, count_out, yolox [T][B][G][5]), a Python loop over the frames."""
    T, B, G, _ = rows.shape
    rows_out, count_out = torch.zeros_like(rows), count.clone()
    yolox = torch.zeros(T, B, G, 5, dtype=rows.dtype, device=rows.device)
    counts = count.tolist()
    for t in range(T):
        for b in range(B):
            n = counts[t][b]
            if n <= 0:
                continue
            lab = labels_frame_ref(rows[t, b, :n], states[b], hw)
            k = lab.shape[0]
            count_out[t, b] = k
            rows_out[t, b, :k] = lab
            yolox[t, b, :k, 0] = lab[:, 5]
            yolox[t, b, :k, 1] = lab[:, 1] + 0.5 * lab[:, 3]
            yolox[t, b, :k, 2] = lab[:, 2] + 0.5 * lab[:, 4]
            yolox[t, b, :k, 3] = lab[:, 3]
            yolox[t, b, :k, 4] = lab[:, 4]
    return rows_out, count_out, yolox
