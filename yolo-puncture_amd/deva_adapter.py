"""`auto_segment` - the one function of the hot path that lives in the reference tree (yolo_seg/yolo_with_deva.py:37-88):
YOLO instance masks -> one int64 id mask + the per-object info list DEVA consumes. Same signature and behaviour; the
per-mask Python loop (`output_mask[mask > 0.5] = curr_id`, :62-86) runs as one GPU pass (yp_masks: GEMM, resize, crop,
threshold, area test, last-painter-wins id paint)."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

import numpy as np
import torch



class ObjectInfo(NamedTuple):
    """Stand-in for deva.inference.object_info.ObjectInfo (external, not vendored): id, score, category_id."""
    id: int
    score: float
    category_id: int


def auto_segment(config: Dict, image: np.ndarray, yolo_model, min_side: int, suppress_small_mask: bool,
                 object_info_cls=ObjectInfo) -> Tuple[torch.Tensor, List]:
    """config: needs .get('MIN_AREA_THRESHOLD', 100); image: uint8 [h,w,3] (fed to YOLO as if BGR, exactly like the
    reference does with its RGB frames - SURVEY Appendix C-6); returns (int64 [h,w] on the model's device, [ObjectInfo])."""
    device = next(yolo_model.model.parameters()).device                     # :42
    h, w = image.shape[:2]
    pre = None
    if min_side > 0:                                                        # :45-48 (cv2.resize default = INTER_LINEAR), done on the GPU
        scale = min_side / min(h, w)
        pre = (int(w * scale), int(h * scale))
    min_area = config.get("MIN_AREA_THRESHOLD", 100) if hasattr(config, "get") else 100
    ids, kept, conf, cls = yolo_model.predict_id_mask(image, conf=0.9, out_hw=(h, w), suppress_small=suppress_small_mask,
                                                      min_area=int(min_area), pre_resize=pre)   # :45-79 fused
    segments_info = []
    kept = kept.tolist()
    for i, k in enumerate(kept):                                            # :82-86 ids consecutive over KEPT masks
        if k > 0:
            segments_info.append(object_info_cls(id=int(k), score=float(conf[i]), category_id=int(cls[i])))
    return ids.to(device), segments_info


def auto_segment_clip(config: Dict, images, yolo_model, min_side: int, suppress_small_mask: bool, object_info_cls=ObjectInfo,
                      batch_size: int = 32) -> List[Tuple[torch.Tensor, List]]:
    """`auto_segment` for the detection frames of a DEVA run, which are known before the run starts (`ti % detection_every == 0` online,
    `num_voting_frames` consecutive frames semi-online; yolo_seg/yolo_with_deva.py:140,197): frames of one shape go through the network
    `batch_size` at a time and through the id-mask tail in one pass per chunk (YOLO.predict_id_mask_clip).
    images: a list of uint8 [h,w,3] arrays of one shape, or a uint8 CUDA tensor [N,h,w,3]; the other arguments as auto_segment.
    -> [(int64 [h,w] id mask on the model's device, [ObjectInfo])] per frame, each equal to auto_segment's result for that frame."""
    if not isinstance(images, torch.Tensor):
        images = list(images)
    if isinstance(images, torch.Tensor):
        hw = tuple(int(v) for v in images.shape[1:3]) if images.dim() == 4 else ()
    else:
        hw = tuple(int(v) for v in np.shape(images[0])[:2]) if len(images) else ()
    pre, out_hw = None, None
    if len(hw) == 2 and min(hw) > 0:                                        # (anything else is refused by predict_id_mask_clip)
        h, w = hw
        out_hw = (h, w)
        if min_side > 0:                                                    # :45-48, as auto_segment
            scale = min_side / min(h, w)
            pre = (int(w * scale), int(h * scale))
    min_area = config.get("MIN_AREA_THRESHOLD", 100) if hasattr(config, "get") else 100
    per_frame = yolo_model.predict_id_mask_clip(images, conf=0.9, out_hw=out_hw, suppress_small=suppress_small_mask, min_area=int(min_area),
                                                pre_resize=pre, batch_size=batch_size)
    if not per_frame:
        return []
    device = next(yolo_model.model.parameters()).device
    out = []
    for ids, kept, conf, cls in per_frame:
        segments_info = [object_info_cls(id=int(k), score=float(conf[i]), category_id=int(cls[i])) for i, k in enumerate(kept.tolist()) if k > 0]
        out.append((ids.to(device), segments_info))
    return out
