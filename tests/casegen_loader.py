"""Deterministic cases of the loader's index rules, so that the golden fixtures (recorded from the reference's
SequenceForRandomAccess / SequenceForIter / ShardedStreamingDataPipe by tests/make_golden_loader.py) store recorded results only.

A sequence case is N windows and the windows its labelled frames end on.  Frames are (2, 12, 16) uint8: every byte of plane 0 of
window w is w + 1 and of plane 1 is 255 - w, so a sample's window range is read back from the data and a padded (all-zero) frame
reads as window -1.  Labelled frame f carries 1 + f % 3 rows whose `t` is 1000 (f + 1): labels are identified from their rows."""
import numpy as np

T = 5
SHAPE = (2, 12, 16)
HW_GEN1 = (240, 304)                                   # the reference's ObjectLabels carry the dataset's frame size

SEQ_CASES = {
    'loader_dense': dict(N=14, o2r=(2, 4, 5, 8, 11)),          # dense labels; first label before window T - 1; N no multiple of T
    'loader_gaps': dict(N=43, o2r=(1, 3, 20, 22, 40)),         # label gaps larger than T: several sub-sequences; offset 2
    'loader_unreachable': dict(N=4, o2r=(1, 3)),               # no label reachable by a T-window sample: random-access length 0
    'loader_single': dict(N=9, o2r=(6,)),                      # a single labelled frame
    'loader_aligned': dict(N=15, o2r=(4, 9, 14)),              # offset 0, N a multiple of T: nothing padded
}

SHARD_LENGTHS = (5, 9, 2, 7, 7, 1, 3)
SHARD_WORLDS = (1, 2, 3)
SHARD_BATCH_SIZES = (1, 2)

LABEL_DTYPE = np.dtype([('t', '<i8'), ('x', '<f4'), ('y', '<f4'), ('w', '<f4'), ('h', '<f4'), ('class_id', 'u1'), ('class_confidence', '<f4')])


def frames(name: str) -> np.ndarray:
    N = SEQ_CASES[name]['N']
    x = np.zeros((N,) + SHAPE, dtype=np.uint8)
    for w in range(N):
        x[w, 0], x[w, 1] = w + 1, 255 - w
    return x


def windows_of(ev: np.ndarray) -> np.ndarray:
    """Window numbers of frames (..., 2, 12, 16) as written by `frames`; -1 for an all-zero (padded) frame."""
    return ev[..., 0, 0, 0].astype(np.int64) - 1


def label_rows(name: str):
    """rows[f]: float32 [n][7] (t x y w h class_id class_confidence) of labelled frame f."""
    out = []
    for f in range(len(SEQ_CASES[name]['o2r'])):
        n = 1 + f % 3
        r = np.zeros((n, 7), dtype=np.float32)
        for i in range(n):
            r[i] = (1000 * (f + 1), 10 + 3 * i + f, 20 + f, 30 + i, 25, (f + i) % 2, 1.0)
        out.append(r)
    return out


def structured_labels(name: str):
    """(labels structured array, objframe_idx_2_label_idx) as the reference's labels_v2/labels.npz holds them."""
    rows = label_rows(name)
    flat = np.concatenate(rows)
    lab = np.zeros(flat.shape[0], dtype=LABEL_DTYPE)
    for k, key in enumerate(LABEL_DTYPE.names):
        lab[key] = flat[:, k]
    idx = np.concatenate(([0], np.cumsum([r.shape[0] for r in rows])[:-1])).astype(np.int64)
    return lab, idx
