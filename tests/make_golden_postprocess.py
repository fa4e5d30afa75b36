"""Golden fixtures of the detection post-processing recorded from the UNMODIFIED reference `postprocess`
(models/detection/yolox/utils/boxes.py:32-76, imported from /root/reference).

TEST INFRASTRUCTURE; runs only in the authoring container and is not collected by pytest.
Usage: python tests/make_golden_postprocess.py

The reference's NMS core is torchvision, which is not installed: oracle/_stubs/torchvision raises from nms / batched_nms.  This
recorder assigns a stand-in onto torchvision.ops at run time - plain greedy NMS on the raw fp32 boxes, per class for batched_nms,
IoU = inter / (area_a + area_b - inter) - and tests/casegen_postprocess.py nudges its data so that the recorded truth does not
depend on the few-ulp differences between this stand-in and the real torchvision kernels.
Stored per case in tests/golden/<case>.npz, for every setting of casegen_postprocess.SETTINGS: count [B] and the concatenated
[n][7] rows.  Only numerical outputs are stored."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle', '_stubs'))
sys.path.insert(1, '/root/reference')
sys.path.insert(2, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torchvision  # noqa: E402  (the stub)

from tests import casegen_postprocess as cg  # noqa: E402


def _greedy(boxes, scores, groups, thr):
    b = boxes.detach().cpu().numpy().astype(np.float32)
    s = scores.detach().cpu().numpy()
    g = groups.detach().cpu().numpy() if groups is not None else np.zeros(len(s))
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = (x2 - x1) * (y2 - y1)
    order = np.argsort(-s, kind='stable')
    alive = np.ones(len(s), dtype=bool)
    keep = []
    for k, i in enumerate(order):
        if not alive[i]:
            continue
        keep.append(i)
        rest = order[k + 1:]
        iw = np.maximum(np.float32(0), np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]))
        ih = np.maximum(np.float32(0), np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]))
        inter = iw * ih
        with np.errstate(divide='ignore', invalid='ignore'):
            iou = inter / (area[i] + area[rest] - inter)
        alive[rest[(iou > np.float32(thr)) & (g[rest] == g[i])]] = False
    return torch.as_tensor(np.asarray(keep, dtype=np.int64))


def nms(boxes, scores, iou_threshold):
    return _greedy(boxes, scores, None, iou_threshold)


def batched_nms(boxes, scores, idxs, iou_threshold):
    return _greedy(boxes, scores, idxs, iou_threshold)


def main():
    torchvision.ops.nms = nms
    torchvision.ops.batched_nms = batched_nms
    from models.detection.yolox.utils.boxes import postprocess
    for name, c in cg.CASES.items():
        pred = cg.make_prediction(name)
        out, kept = {}, {}
        for s in cg.SETTINGS:
            conf, thr, agn = s
            res = postprocess(torch.from_numpy(pred.copy()), c['nc'], conf_thre=conf, nms_thre=thr, class_agnostic=agn)
            counts = np.array([0 if r is None else r.shape[0] for r in res], dtype=np.int32)
            rows = [r.numpy().astype(np.float32) for r in res if r is not None]
            out[f'{cg.setting_id(s)}/count'] = counts
            out[f'{cg.setting_id(s)}/rows'] = np.concatenate(rows) if rows else np.zeros((0, 7), dtype=np.float32)
            kept[s] = counts.tolist()
            print(f'{name} {cg.setting_id(s)}: candidates {cg.candidate_counts(name, conf)} kept {kept[s]}')
        cg.check_results(name, kept)
        print(f'{name}: nudged {cg.nudged(name)} of {pred.shape[0] * pred.shape[1]} anchors')
        np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', f'{name}.npz'), **out)


if __name__ == '__main__':
    main()
