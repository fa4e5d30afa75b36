"""rvt_render_preview (rvt_amd/csrc/capi_viz.hip, rvt_amd/viz.py): event planes and box lists to RGB preview images.  Every
comparison is np.array_equal on the whole output: the feature has no tolerance.  The yardsticks are not the code under test: the
numpy restatement of the rule (tests/viz_ref.py) paints box after box, and tests/golden/viz_evimg.npz holds what the reference's own
`ev_repr_to_img` returned (tests/make_golden_viz.py).  Shapes are the smallest at which an edge can go wrong: one pixel, a width
below, at and above the 16-pixel piece, two row chunks of one image (70 x 33), more pieces than threads (1 x 4112), more boxes than
one scan tile (300)."""
import functools
import os

import numpy as np
import pytest
import torch

import opmodel
from rvt_amd import _header, _lib, viz
from rvt_amd.types import DataType
from tests import viz_ref as ref
from tests.backends import backend  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'viz_evimg.npz')
CANARY = 0x5A
GLYPHS = viz.glyph_table()
PALETTE = {d: np.array(viz.PALETTES[d], dtype=np.uint8) for d in viz.PALETTES}
NAMES = {d: viz.name_table(viz.LABELMAPS[d]) for d in viz.LABELMAPS}
NAN, INF = float('nan'), float('inf')


@functools.lru_cache(maxsize=None)
def _planes(F, C, H, W, dtype):
    """Sparse event planes with every sign of the difference, sums that cancel and, for int8, a plane of -128."""
    rng = np.random.default_rng(1000 * H + 10 * W + C + (dtype == 'int8'))
    lo, hi = (0, 6) if dtype == 'uint8' else (-4, 5)
    x = (rng.integers(lo, hi, size=(F, C, H, W)) * (rng.random((F, C, H, W)) < 0.35)).astype(dtype)
    x[:, :, 0, 0] = 3                                    # both halves equal: grey
    if dtype == 'int8':
        x[:, 0, H - 1, W - 1] = -128                     # first half far below: white
        x[:, :, H // 2, W // 2] = -128                   # cancels
    else:
        x[:, :, H - 1, W - 1] = 255                      # 255 * C / 2 on either side
    x.setflags(write=False)
    return x


def _det(boxes, N=None):
    """[(x1, y1, x2, y2, score, cls)] per frame -> rows fp32 [F][N][7], count int32 [F]."""
    N = max([len(b) for b in boxes] + [1]) if N is None else N
    rows = np.zeros((len(boxes), N, 7), dtype=np.float32)
    for f, bs in enumerate(boxes):
        for j, (x1, y1, x2, y2, s, c) in enumerate(bs[:N]):
            rows[f, j] = (x1, y1, x2, y2, 0.9, s, c)
    return rows, np.array([len(b) for b in boxes], dtype=np.int32)


def _lab(boxes, N=None):
    """[(x, y, w, h, cls)] per frame (None: a frame without labels) -> rows fp32 [F][N][7], count int32 [F] with -1."""
    N = max([len(b) for b in boxes if b is not None] + [1]) if N is None else N
    rows = np.zeros((len(boxes), N, 7), dtype=np.float32)
    for f, bs in enumerate(boxes):
        for j, (x, y, w, h, c) in enumerate((bs or [])[:N]):
            rows[f, j] = (1e5 + f, x, y, w, h, c, 1.0)
    return rows, np.array([-1 if b is None else len(b) for b in boxes], dtype=np.int32)


def _run(dev, planes, det=None, lab=None, frame_index=None, scale=1, text=True, dataset='gen1', palette=None, names=None, offset=0,
         lead=None):
    """render_preview into a canary-filled buffer at a byte offset; returns (image [Fout][P*Hs][Ws][3] as numpy, status)."""
    F, C, H, W = planes.shape
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)                  # noqa: E731
    shp = lambda a, tail: a if lead is None else a.reshape(lead + tail)                           # noqa: E731
    P = max((det is not None) + (lab is not None), 1)
    Fout = F if frame_index is None else len(frame_index)
    shape = (Fout, P * H * scale, W * scale, 3)
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), CANARY, dtype=torch.uint8, device=dev)
    base = (-buf.data_ptr()) % 16 + offset               # offset 0 and 16: 16-byte aligned, 1: not
    out = buf[base:base + n].view(shape)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = {}
    if det is not None:
        kw.update(det=t(shp(det[0], det[0].shape[1:])), det_count=t(shp(det[1], ())))
    if lab is not None:
        kw.update(label_rows=t(shp(lab[0], lab[0].shape[1:])), label_count=t(shp(lab[1], ())))
    got = viz.render_preview(t(shp(planes, (C, H, W))), frame_index=None if frame_index is None else t(np.asarray(frame_index, dtype=np.int64)),
                             dataset=dataset, palette=None if palette is None else t(np.asarray(palette, dtype=np.uint8)), names=names, scale=scale, text=text, out=out, status=status, **kw)
    assert got is out
    host = buf.cpu().numpy()
    assert (host[:base] == CANARY).all() and (host[base + n:] == CANARY).all(), 'bytes outside out were written'
    return host[base:base + n].reshape(shape), int(status.cpu()[0])


def _want(planes, det=None, lab=None, frame_index=None, scale=1, text=True, dataset='gen1', palette=None, names=None):
    panels = [(d[0], d[1], k) for d, k in ((det, ref.KIND_DET), (lab, ref.KIND_LABEL)) if d is not None] or [None]
    pal = PALETTE[dataset] if palette is None else np.asarray(palette, dtype=np.uint8)
    nam = NAMES[dataset] if names is None else viz.name_table(names)
    img, status = ref.render(planes, panels, pal, nam, GLYPHS, frame_index=frame_index, scale=scale, text=text)
    Fo, P, Hs, Ws, _ = img.shape
    return img.reshape(Fo, P * Hs, Ws, 3), status


def _check(dev, planes, **kw):
    offset, lead = kw.pop('offset', 0), kw.pop('lead', None)
    got, st = _run(dev, planes, offset=offset, lead=lead, **kw)
    want, wst = _want(planes, **kw)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f'{int((got != want).any(axis=-1).sum())} pixels differ'
    assert st == wst
    return got


# ---- 1. the base image -----------------------------------------------------------------------------------------------------------------
def test_glyph_table_is_well_formed():
    assert GLYPHS.shape == (128, 7) and GLYPHS.dtype == np.uint8 and (GLYPHS < 32).all()
    for ch in 'carpedestrian two wheeler0123456789.':
        assert (GLYPHS[ord(ch)].any()) == (ch != ' '), ch
    assert all(len(v) == 14 for v in viz._GLYPHS.values())


def test_ev_repr_to_img_matches_the_reference_function(backend):
    """The recorded inputs and outputs of the reference's unmodified VizCallbackBase.ev_repr_to_img."""
    g = np.load(GOLDEN)
    names = sorted(k[3:] for k in g.files if k.startswith('in_'))
    assert names == ['i8_c10', 'u8_c2', 'u8_c20']
    for name in names:
        x, want = g['in_' + name], g['out_' + name]
        got = viz.ev_repr_to_img(torch.from_numpy(x[None]).to(backend)).cpu().numpy()
        assert got.shape == (1,) + want.shape and np.array_equal(got[0], want), name
        assert np.array_equal(ref.base_image(x), want), name             # the restatement is held to the same record
        assert {0, 127, 255} == set(np.unique(want)) or name == 'u8_c2'


@pytest.mark.parametrize('dtype', ['uint8', 'int8'])
@pytest.mark.parametrize('C', [2, 20])
@pytest.mark.parametrize('hw', [(1, 1), (3, 5), (12, 16), (7, 33), (24, 48)], ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_base_image(backend, hw, C, dtype):
    x = _planes(2, C, hw[0], hw[1], dtype)
    got = _check(backend, x, text=False)
    assert np.array_equal(got[:, 0, 0], np.full((2, 3), 127))            # the sums cancel


def test_base_image_more_pieces_than_threads_and_two_chunks(backend):
    _check(backend, _planes(1, 2, 1, 4112, 'uint8'), text=False)
    _check(backend, _planes(1, 2, 1, 4100, 'int8'), text=False)
    _check(backend, _planes(2, 4, 70, 33, 'uint8'), text=False)


# ---- 2. scale and alignment ----------------------------------------------------------------------------------------------------------------
BOXES_48 = [[(3.2, 12.7, 20.9, 22.1, 0.87, 0), (30, 2, 47.5, 23.5, 0.4, 1)], [(10, 10, 30, 20, 0.5, 1)]]
LABELS_48 = [[(5, 11, 12, 9, 1)], None]


@pytest.mark.parametrize('offset', [0, 1, 16])
@pytest.mark.parametrize('scale', [1, 2, 4])
@pytest.mark.parametrize('hw', [(24, 48), (7, 33)], ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_scale_and_alignment(backend, hw, scale, offset):
    x = _planes(2, 20, hw[0], hw[1], 'uint8')
    _check(backend, x, det=_det(BOXES_48), lab=_lab(LABELS_48), scale=scale, offset=offset)


# ---- 3. frame index ----------------------------------------------------------------------------------------------------------------------------
def test_frame_index(backend):
    x = _planes(3, 2, 12, 16, 'uint8')
    det = _det([[(1, 1, 8, 8, 0.5, 0)], [(2, 3, 12, 10, 0.25, 1)], []])
    lab = _lab([None, [(4, 1, 5, 9, 0)], [(0, 0, 15, 11, 1)]])
    for idx, bit in (([2, 0, 1], 0), ([1, 1, 1, 0], 0), ([0, -1, 2], 0), ([0, 3, 1], 1), ([-2, 0], 1), ([-1], 0)):
        got, st = _run(backend, x, det=det, lab=lab, frame_index=idx)
        want, wst = _want(x, det=det, lab=lab, frame_index=idx)
        assert np.array_equal(got, want), idx
        assert st == wst == bit, idx
        for i, f in enumerate(idx):
            if not 0 <= f < 3:
                assert not got[i].any(), idx


def test_time_batch_form(backend):
    x = _planes(6, 20, 12, 16, 'int8')
    det = _det([[(f, 1, 8 + f, 9, 0.1 * f, f % 2)] for f in range(6)])
    lab = _lab([[(2, f, 6, 5, 1)] if f % 2 else None for f in range(6)])
    flat = _check(backend, x, det=det, lab=lab)
    tb = _check(backend, x, det=det, lab=lab, lead=(3, 2))
    assert np.array_equal(flat, tb)
    _check(backend, x, det=det, lab=lab, lead=(3, 2), frame_index=[5, 0, -1])


# ---- 4. boxes --------------------------------------------------------------------------------------------------------------------------------
H4, W4 = 24, 48
BOX_CASES = {
    'none': [],
    'outside_left': [(-30, 5, -20, 15, 0.5, 0)], 'outside_right': [(60, 5, 70, 15, 0.5, 0)],
    'outside_top': [(5, -40, 15, -30, 0.5, 0)], 'outside_bottom': [(5, 40, 15, 50, 0.5, 0)],
    'straddle_left': [(-5, 5, 10, 15, 0.5, 0)], 'straddle_right': [(40, 5, 55, 15, 0.5, 1)],
    'straddle_top': [(5, -5, 15, 8, 0.5, 0)], 'straddle_bottom': [(5, 18, 15, 30, 0.5, 1)],
    'negative_half': [(-0.5, -0.5, 10.5, 12.5, 0.5, 0)],
    'w0': [(7, 12, 7, 20, 0.5, 0)], 'h0': [(7, 12, 20, 12, 0.5, 1)], 'w0_h0': [(30, 15, 30, 15, 0.5, 0)],
    'whole_image': [(0, 0, W4 - 1, H4 - 1, 0.5, 1)],
    'overlap_ab': [(4, 10, 30, 20, 0.5, 0), (10, 12, 40, 22, 0.6, 1)],
    'overlap_ba': [(10, 12, 40, 22, 0.6, 1), (4, 10, 30, 20, 0.5, 0)],
    'class_beyond_palette': [(4, 10, 30, 20, 0.5, 5)],
    'class_minus_one': [(4, 10, 30, 20, 0.5, -1), (6, 12, 20, 18, 0.5, 0)],
    'negative_extent': [(20, 10, 10, 20, 0.5, 0), (10, 20, 20, 10, 0.5, 0), (3, 11, 9, 17, 0.5, 1)],
}


@pytest.mark.parametrize('case', sorted(BOX_CASES))
def test_boxes(backend, case):
    x = _planes(1, 2, H4, W4, 'uint8')
    xywh = [[(x1, y1, x2 - x1, y2 - y1, c) for x1, y1, x2, y2, _, c in BOX_CASES[case]]]
    got = _check(backend, x, det=_det([BOX_CASES[case]]), lab=_lab(xywh))
    if case.startswith('outside') or case == 'none':                                     # no outline pixel (a tag may still reach in)
        bare = _check(backend, x, det=_det([BOX_CASES[case]]), lab=_lab(xywh), text=False)
        assert np.array_equal(bare, _want(x, det=_det([[]]), lab=_lab([None]))[0])
    if case == 'overlap_ab':
        other = _check(backend, x, det=_det([BOX_CASES['overlap_ba']]), lab=_lab([[xywh[0][1], xywh[0][0]]]))
        assert not np.array_equal(got, other)                                            # the order shows


def test_label_count_minus_one_and_det_count_above_max_det(backend):
    x = _planes(2, 2, H4, W4, 'uint8')
    det = _det([[(2, 10, 12, 20, 0.5, 0), (14, 10, 24, 20, 0.5, 1), (26, 10, 36, 20, 0.5, 0)]] * 2, N=2)
    assert det[0].shape[1] == 2 and det[1].tolist() == [3, 3]            # count is the number kept before the cap
    lab = _lab([None, [(3, 3, 4, 4, 0)]])
    got = _check(backend, x, det=det, lab=lab)
    assert np.array_equal(got[0, H4:], ref.base_image(x[0]))             # count -1: the label panel is the base image


@pytest.mark.parametrize('field', range(5))
@pytest.mark.parametrize('bad', [NAN, INF, 3e6], ids=['nan', 'inf', '3e6'])
def test_unpaintable_numbers_skip_the_box(backend, field, bad):
    """NaN, +inf and 3e6 in each of the five fields: the box is skipped, its neighbours are drawn, nothing faults."""
    x = _planes(1, 2, H4, W4, 'uint8')
    d = [4.0, 10.0, 30.0, 20.0, 0.5, 1.0]
    d[(0, 1, 2, 3, 5)[field]] = bad
    lb = [4.0, 10.0, 26.0, 10.0, 1.0]
    lb[field] = bad
    good = (6, 12, 20, 18, 0.5, 0)
    got = _check(backend, x, det=_det([[good, tuple(d), (33, 12, 44, 20, 0.7, 1)]]), lab=_lab([[(6, 12, 14, 6, 0), tuple(lb)]]))
    want = _want(x, det=_det([[good, (33, 12, 44, 20, 0.7, 1)]]), lab=_lab([[(6, 12, 14, 6, 0)]]))[0]
    assert np.array_equal(got, want)
    # -inf too, and two infinities whose difference is NaN
    _check(backend, x, det=_det([[(INF, 1, INF, 9, 0.5, 0), (1, -INF, 9, 5, 0.5, 0), good]]), lab=_lab([[(1, 2, -INF, 4, 0)]]))


def test_more_boxes_than_a_scan_tile_and_more_than_the_cap(backend):
    rng = np.random.default_rng(5)

    def boxes(n):
        x1, y1 = rng.integers(-8, 40, n), rng.integers(-8, 70, n)
        return [(int(a), int(b), int(a + w), int(b + h), float(s), int(c))
                for a, b, w, h, s, c in zip(x1, y1, rng.integers(0, 20, n), rng.integers(0, 20, n), rng.random(n), rng.integers(0, 3, n))]
    x = _planes(2, 4, 70, 33, 'uint8')
    _check(backend, x, det=_det([boxes(300), boxes(7)]), text=False)
    _check(backend, x, det=_det([boxes(40), boxes(300)]), dataset='gen4')
    many = boxes(520)                                                    # rows behind the first 512 are not drawn
    got = _check(backend, x[:1], det=_det([many]), text=False)
    assert np.array_equal(got, _want(x[:1], det=_det([many[:512]]), text=False)[0])


# ---- 5. tags ---------------------------------------------------------------------------------------------------------------------------------
def test_tags(backend):
    x = _planes(1, 2, H4, W4, 'uint8')
    above = _check(backend, x, det=_det([[(2, 12, 20, 20, 0.87, 0)]]))                   # y0 - 9 >= 0: above the box
    inside = _check(backend, x, det=_det([[(2, 8, 20, 20, 0.87, 0)]]))                   # pushed inside at the top border
    yellow, blue = PALETTE['gen1']
    assert (above[0, 3:12, 2] == yellow).all() and (inside[0, 9:18, 2] == yellow).all() and not (inside[0, 0:8, 2] == yellow).all()
    assert (above[0, 4:11, 3:8] == 0).all(axis=-1).any()                 # black ink on yellow
    white = _check(backend, x, det=_det([[(2, 12, 20, 20, 0.87, 1)]]))
    assert (white[0, 4:11, 3:8] == 255).all(axis=-1).any() and (white[0, 3, 2] == blue).all()    # white ink on blue
    _check(backend, x, det=_det([[(30, 12, 46, 20, 0.5, 0)]]), lab=_lab([[(40, 12, 5, 5, 1)]]))  # clipped at the right border
    _check(backend, x, det=_det([[(-20, 12, 46, 20, 0.5, 1)]]), lab=_lab([[(-7, 12, 15, 5, 0)]]))  # ... and at the left one
    _check(backend, x, det=_det([[(2, 9, 20, 20, 0.5, 0)]]))                             # y0 = 9: the tag's top row is row 0


@pytest.mark.parametrize('score,digits', [(0.0, '0.00'), (0.005, '0.01'), (0.994999, '0.99'), (0.995, '1.00'), (1.0, '1.00'),
                                          (-3.0, '0.00'), (7.5, '1.00')])
def test_tag_scores(backend, score, digits):
    assert ref.score_digits(np.float32(score)) == digits
    x = _planes(1, 2, 12, 80, 'uint8')
    _check(backend, x, det=_det([[(1, 10, 70, 11, score, 1)]]))


def test_names_palettes_and_an_empty_glyph(backend):
    x = _planes(1, 2, H4, 112, 'uint8')
    names = ['a~b', 'Truck 7', '', 'twelve chars', 'thirteen chars']             # '~' has no glyph; 12 fill the row; 14 are cut
    assert not GLYPHS[ord('~')].any() and viz.name_table(names)[4].tobytes() == b'thirteen cha'
    pal = [(255, 0, 0), (10, 200, 40), (200, 100, 83), (200, 100, 84), (0, 0, 0)]  # r + g + b = 383 and 384: white and black ink
    det = _det([[(1, 10, 30, 12, 0.5, 0), (50, 10, 90, 12, 0.25, 1), (1, 22, 30, 23, 0.75, 2), (40, 22, 111, 23, 1.0, 3)]])
    lab = _lab([[(1, 10, 30, 2, 2), (8, 22, 30, 1, 3), (60, 10, 3, 3, 4), (5, 3, 2, 2, 9)]])
    for text in (True, False):
        _check(backend, x, det=det, lab=lab, palette=pal, names=names, text=text)
    _check(backend, x, det=det, lab=lab, dataset='gen4', scale=2)


# ---- 6. panels, determinism, the helper, files, pricing ----------------------------------------------------------------------------------
def test_two_panels_are_the_single_panels_stacked(backend):
    x = _planes(2, 20, 7, 33, 'int8')
    det, lab = _det([[(3, 1, 20, 5, 0.3, 0)], [(0, 0, 32, 6, 0.6, 1)]]), _lab([[(2, 2, 9, 3, 1)], None])
    both = _check(backend, x, det=det, lab=lab, scale=2)
    top, bottom = _check(backend, x, det=det, scale=2), _check(backend, x, lab=lab, scale=2)
    assert np.array_equal(both, np.concatenate([top, bottom], axis=1))
    again, _ = _run(backend, x, det=det, lab=lab, scale=2)
    assert np.array_equal(both, again)                                   # two calls, equal bytes
    plain = viz.ev_repr_to_img(torch.from_numpy(x.copy()).to(backend)).cpu().numpy()
    assert np.array_equal(plain, _want(x, text=False)[0])


def test_argument_checks(backend):
    dev = backend
    x = torch.zeros(2, 4, 6, 16, dtype=torch.uint8, device=dev)
    rows, count = torch.zeros(2, 3, 7, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError, match='planes must be uint8 or int8'):
        viz.render_preview(x.float())
    with pytest.raises(ValueError, match='even number of channels'):
        viz.render_preview(x[:, :3].contiguous())
    with pytest.raises(ValueError, match='planes must be contiguous'):
        viz.render_preview(x[:, :, :, ::2])
    with pytest.raises(ValueError, match='scale must be one of'):
        viz.render_preview(x, scale=3)
    with pytest.raises(ValueError, match='det rows without det_count'):
        viz.render_preview(x, det=rows)
    with pytest.raises(TypeError, match=r'det rows must be float32 \[2\]\[N\]\[7\]'):
        viz.render_preview(x, det=rows[:1], det_count=count)
    with pytest.raises(TypeError, match=r'label count must be int32 \[2\]'):
        viz.render_preview(x, label_rows=rows, label_count=count.long())
    with pytest.raises(TypeError, match='frame_index must be int64'):
        viz.render_preview(x, frame_index=count)
    with pytest.raises(ValueError, match='out must be contiguous uint8'):
        viz.render_preview(x, out=torch.zeros(2, 6, 16, 4, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='dataset must be one of'):
        viz.render_preview(x, dataset='gen9')
    lib = _lib.get_lib()                                                 # the C side refuses what the Python side cannot build
    args = [x.data_ptr(), 0, 2, 4, 6, 16, None, None, 0, 0, None, None, 0, 0, 1, None, 2, x.data_ptr(), 1, None, 0, None, 1, 0,
            x.data_ptr(), count.data_ptr(), None]
    for pos, val, says in ((22, 3, 'scale=3'), (14, 3, 'P=3'), (3, 5, 'C=5'), (16, 3, 'Fout=3 must not exceed F=2'), (23, 1, 'RVT_VIZ_TEXT needs names')):
        bad = list(args)
        bad[pos] = val
        assert lib.rvt_render_preview(*bad) != 0 and says in lib.rvt_last_error().decode(), says


def _loader_batch(dev, T=3, B=2, G=4):
    rng = np.random.default_rng(11)
    ev = torch.from_numpy(_planes(T * B, 20, 12, 16, 'uint8').reshape(T, B, 20, 12, 16).copy()).to(dev)
    boxes = [[(1 + f, 2, 6, 5, f % 2)] if f in (0, 1, 3, 4) else None for f in range(T * B)]
    rows, count = _lab(boxes, N=G)
    labelled = torch.from_numpy(count.reshape(T, B) > 0).to(dev)
    det = _det([[(int(rng.integers(0, 8)), 1, 12, 9, 0.5, f % 2)] for f in range(T * B)], N=5)
    batch = {'data': {DataType.EV_REPR: ev}, 'worker_id': 0,
             'device_labels': (torch.from_numpy(rows.reshape(T, B, G, 7)).to(dev), torch.from_numpy(count.reshape(T, B)).to(dev), None, labelled)}
    return batch, ev.cpu().numpy().reshape(T * B, 20, 12, 16), (rows, count), det


def test_detection_preview_picks_the_last_labelled_frames(backend, tmp_path):
    T, B = 3, 2
    batch, planes, lab, det = _loader_batch(backend, T, B)
    dt = (torch.from_numpy(det[0].reshape(T, B, 5, 7)).to(backend), torch.from_numpy(det[1].reshape(T, B)).to(backend))
    # the restated rule (callbacks/detection.py:48-51): the step's labelled frames in (t, b) order, the last n of them, last first
    labelled = [f for f in range(T * B) if lab[1][f] > 0]
    assert labelled == [0, 1, 3, 4]
    for n, want_idx in ((2, [4, 3]), (4, [4, 3, 1, 0]), (6, [4, 3, 1, 0, -1, -1])):
        assert viz.last_labelled(batch['device_labels'][3], n).cpu().tolist() == want_idx
        assert want_idx[:len(labelled)] == labelled[::-1][:n]
    pv = viz.DetectionPreview('gen1', n_samples=3, every_n_steps=10)
    assert pv.on_train_batch(5, batch, *dt) is None and pv.images() == []
    img = pv.on_train_batch(20, batch, *dt)
    want, _ = _want(planes, det=det, lab=lab, frame_index=[4, 3, 1])
    assert img.device.type == backend.type and np.array_equal(img.cpu().numpy(), want)
    (step, kept), = pv.images()
    assert step == 20 and kept is img
    labels_only = viz.DetectionPreview('gen1', n_samples=1, every_n_steps=1).on_train_batch(0, batch)
    assert np.array_equal(labels_only.cpu().numpy(), _want(planes, lab=lab, frame_index=[4])[0])

    # files: binary PPM through a parser written here
    files = pv.save(str(tmp_path / 'previews'))
    ppm = sorted(f for f in files if f.endswith('.ppm'))
    assert [os.path.basename(f) for f in ppm] == [f'step00000020_{i}.ppm' for i in range(3)]
    for i, f in enumerate(ppm):
        assert np.array_equal(_read_ppm(f), want[i])
    try:
        from PIL import Image
    except ImportError:
        assert len(files) == 3
    else:
        assert len(files) == 6 and np.array_equal(np.asarray(Image.open(ppm[0][:-4] + '.png')), want[0])


def _read_ppm(path):
    with open(path, 'rb') as f:
        data = f.read()
    fields, pos = [], 0
    while len(fields) < 4:                                               # magic, width, height, maxval: whitespace separated
        while data[pos:pos + 1].isspace():
            pos += 1
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        fields.append(data[pos:end])
        pos = end
    assert fields[0] == b'P6' and fields[3] == b'255'
    w, h = int(fields[1]), int(fields[2])
    body = data[pos + 1:]                                                # one whitespace byte behind maxval
    assert len(body) == w * h * 3
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w, 3)


def test_opmodel_prices_a_recorded_launch(backend):
    x = _planes(3, 20, 12, 16, 'uint8')
    calls, orig = [], _lib.call

    def rec(name, *args):
        calls.append((name, args))
        return orig(name, *args)
    _lib.call = rec
    try:
        _run(backend, x, det=_det([[(1, 1, 5, 5, 0.5, 0)]] * 3), lab=_lab([None] * 3), frame_index=[2, 0], scale=2)
    finally:
        _lib.call = orig
    (name, args), = calls
    assert name == 'rvt_render_preview'
    assert _header.PROTOS[name].argnames == (
        'planes', 'planes_signed', 'F', 'C', 'H', 'W', 'rows0', 'count0', 'N0', 'kind0', 'rows1', 'count1', 'N1', 'kind1', 'P',
        'frame_index', 'Fout', 'palette', 'n_palette', 'names', 'n_names', 'glyphs', 'scale', 'flags', 'out', 'status', 'stream')
    want = 2 * 20 * 12 * 16 + 2 * 2 * 24 * 32 * 3
    assert opmodel.render_preview_bytes(2, 20, 12, 16, 2, 2) == want
    assert opmodel.model(name, args) == (0.0, float(want)) and opmodel.executed(name, args) == 0.0


# ---- 7. graph capture (the device only) ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_after_rewriting_the_inputs_in_place():
    _lib._install_test_library(None)
    dev = torch.device('cuda', 0)
    xa, xb = _planes(3, 20, 24, 48, 'uint8'), _planes(3, 20, 24, 48, 'uint8')[::-1].copy()
    da, db = _det([[(3, 12, 20, 22, 0.87, 0)], [], [(30, 2, 47, 23, 0.4, 1)]], N=2), _det([[], [(1, 10, 9, 18, 0.1, 1), (5, 5, 40, 20, 0.6, 0)], []], N=2)
    la, lb = _lab([[(5, 11, 12, 9, 1)], None, None], N=2), _lab([None, [(0, 0, 47, 23, 0)], [(9, 9, 9, 9, 1)]], N=2)
    ia, ib = [2, 0, 1, -1], [1, 1, 0, 2]
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)                  # noqa: E731
    planes, rows, cnt, lrows, lcnt, idx = t(xa), t(da[0]), t(da[1]), t(la[0]), t(la[1]), t(np.asarray(ia, dtype=np.int64))
    out = torch.empty(4, 2 * 24 * 2, 48 * 2, 3, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    call = lambda: viz.render_preview(planes, rows, cnt, lrows, lcnt, frame_index=idx, scale=2, out=out, status=status)   # noqa: E731
    call()                                                               # warm-up: the device tables exist before the capture
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _want(xa, det=da, lab=la, frame_index=ia, scale=2)[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for src, dst in ((xb, planes), (db[0], rows), (db[1], cnt), (lb[0], lrows), (lb[1], lcnt), (np.asarray(ib, dtype=np.int64), idx)):
        dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.cpu().numpy().copy()
    eager = viz.render_preview(t(xb), t(db[0]), t(db[1]), t(lb[0]), t(lb[1]), frame_index=t(np.asarray(ib, dtype=np.int64)), scale=2)
    assert np.array_equal(replayed, eager.cpu().numpy())
    assert np.array_equal(replayed, _want(xb, det=db, lab=lb, frame_index=ib, scale=2)[0])
