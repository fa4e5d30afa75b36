"""rvt_amd — MI355X (gfx950)-native recurrent-vision-transformer backbone (hot path of uzh-rpg/RVT)."""
from .backbone import RNNDetector, RNNDetectorStage, build_recurrent_backbone  # noqa: F401
from .config import AttrDict, backbone_config, modify_backbone_config  # noqa: F401
from .detector import YoloXDetector  # noqa: F401,E402  (backbone + PAFPN + head: the reference's detector class, native)
from .postprocess import postprocess, postprocess_padded  # noqa: F401,E402  (detection post-processing: score filter + batched NMS)
from .evaluation import DetectionEvaluator, PropheseeEvaluator  # noqa: F401,E402  (Prophesee / COCO mAP of the detections, on the device)
from . import optim  # noqa: F401,E402  (optimizer step on the device: value clip + AdamW + OneCycleLR in one launch)
from . import framecache  # noqa: F401,E402  (sparse frame cache: event tensors packed on the device, unpacked by frame index)
from .framecache import FrameGather, PackedFrames, PackedFrames2, gather_frames, pack_frames, unpack_augment, unpack_frames  # noqa: F401,E402
from . import loader  # noqa: F401,E402  (epoch loader over the frame cache: sequences, samplers, batches for the step)
from .loader import BatchLoader, SequenceStore, SparseLabels  # noqa: F401,E402
from . import viz  # noqa: F401,E402  (detection previews: event frames and boxes to RGB images, one launch)
from .viz import DetectionPreview, ev_repr_to_img, render_preview  # noqa: F401,E402
