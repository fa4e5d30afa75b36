"""numpy restatement of the rendering rule of rvt_render_preview (include/rvt_hip.h), for tests/test_viz.py.

Deliberately NOT the kernel's per-pixel search: every image starts as the base image and box after box is painted into it in row
order, outline first, then the tag, later paint covering earlier.  Plain Python loops over boxes and characters, numpy slices for
the rectangles."""
import numpy as np

KIND_DET, KIND_LABEL = 0, 1
MAX_BOXES = 512
LIMIT = np.float32(2.0 ** 20)


def base_image(frame: np.ndarray) -> np.ndarray:
    """frame [C][H][W] uint8 or int8 -> uint8 [H][W][3]."""
    C = frame.shape[0]
    assert C >= 2 and C % 2 == 0
    v = frame.astype(np.int32)
    d = v[C // 2:].sum(axis=0) - v[:C // 2].sum(axis=0)
    img = np.full(d.shape + (3,), 127, dtype=np.uint8)
    img[d > 0] = 255
    img[d < 0] = 0
    return img


def box_of(row: np.ndarray, kind: int):
    """(x0, y0, x1, y1, cls, score) of one fp32 row, or None when the box is skipped."""
    row = row.astype(np.float32)
    with np.errstate(all='ignore'):
        if kind == KIND_DET:
            x, y, w, h, score, cls = row[0], row[1], np.float32(row[2] - row[0]), np.float32(row[3] - row[1]), row[5], row[6]
        else:
            x, y, w, h, cls, score = row[1], row[2], row[3], row[4], row[5], None
        five = (x, y, w, h, cls)
        if any(not np.isfinite(v) or abs(v) >= LIMIT for v in five):
            return None
    if w < 0 or h < 0 or cls < 0:
        return None
    x0, y0 = int(x), int(y)
    return x0, y0, x0 + int(w), y0 + int(h), int(cls), score


def score_digits(score) -> str:
    with np.errstate(all='ignore'):
        if not np.isfinite(score):
            q = 100 if score == np.inf else 0
        else:
            t = np.float32(np.float32(np.float32(score) * np.float32(100.0)) + np.float32(0.5))
            q = 100 if t >= 100 else (0 if t <= 0 else int(t))
    return f'{q // 100}.{q // 10 % 10}{q % 10}'


def fill(img: np.ndarray, xa: int, ya: int, xb: int, yb: int, colour) -> None:
    """The inclusive rectangle [xa, xb] x [ya, yb], clipped to the image."""
    H, W = img.shape[:2]
    xa, ya, xb, yb = max(xa, 0), max(ya, 0), min(xb, W - 1), min(yb, H - 1)
    if xa <= xb and ya <= yb:
        img[ya:yb + 1, xa:xb + 1] = colour


def paint_box(img: np.ndarray, box, kind: int, palette: np.ndarray, names: np.ndarray, glyphs: np.ndarray, text: bool) -> None:
    x0, y0, x1, y1, cls, score = box
    colour = palette[cls % len(palette)]
    fill(img, x0, y0, x1, y0, colour)
    fill(img, x0, y1, x1, y1, colour)
    fill(img, x0, y0, x0, y1, colour)
    fill(img, x1, y0, x1, y1, colour)
    if not text:
        return
    name = names[cls % len(names)]
    zero = np.flatnonzero(name == 0)
    chars = [int(c) for c in name[:zero[0] if len(zero) else len(name)]]
    if kind == KIND_DET:
        chars += [ord(c) for c in ' ' + score_digits(score)]
    ty = y0 - 9 if y0 - 9 >= 0 else y0 + 1
    fill(img, x0, ty, x0 + 6 * len(chars), ty + 8, colour)
    ink = (0, 0, 0) if int(colour[0]) + int(colour[1]) + int(colour[2]) >= 384 else (255, 255, 255)
    for i, ch in enumerate(chars):
        for gy in range(7):
            bits = int(glyphs[ch & 127][gy])
            for gx in range(5):
                if bits >> (4 - gx) & 1:
                    px, py = x0 + 1 + 6 * i + gx, ty + 1 + gy
                    fill(img, px, py, px, py, ink)


def render(planes: np.ndarray, panels, palette: np.ndarray, names: np.ndarray, glyphs: np.ndarray, frame_index=None, scale: int = 1,
           text: bool = True):
    """planes [F][C][H][W]; panels: one or two of (rows [F][N][7], count [F], kind) or None (a panel without boxes).
    Returns (uint8 [Fout][P][Hs][Ws][3], status)."""
    F, _, H, W = planes.shape
    index = np.arange(F) if frame_index is None else np.asarray(frame_index)
    out = np.zeros((len(index), len(panels), H * scale, W * scale, 3), dtype=np.uint8)
    status = 0
    for i, f in enumerate(index):
        if f == -1:
            continue
        if f < 0 or f >= F:
            status |= 1
            continue
        base = base_image(planes[f])
        for p, panel in enumerate(panels):
            img = base.copy()
            if panel is not None:
                rows, count, kind = panel
                n = max(0, min(int(count[f]), rows.shape[1], MAX_BOXES))
                for j in range(n):
                    box = box_of(rows[f, j], kind)
                    if box is not None:
                        paint_box(img, box, kind, palette, names, glyphs, text)
            out[i, p] = img.repeat(scale, axis=0).repeat(scale, axis=1)
    return out, status
