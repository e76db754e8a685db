"""EfficientNet-B3 needle classifier on the MI355X engine: host mirror of the reference's `load_classify_net` / `predict_images` /
`predict_and_find_start_inserted` / `fix_class_prob` (yolo_seg/tasks/needle_clasify.py:41-199, called from yolo_seg/app.py:116-123)
over libyolop.so's yp_cls_* entry points.

The network is efficientnet_pytorch's `EfficientNet.from_name('efficientnet-b3', num_classes=2)` (yolo_seg/tasks/models/efficientnet.py):
26 MBConv blocks with squeeze-excitation, TF "SAME" static padding computed for the configured image size 300, eval-mode BatchNorm
with eps 1e-3. It runs only through the HIP library: the 380x380 crop window is read on the device straight from
the uint8 frame; there is no CPU fallback. The insertion-frame search and the sequence repair are host logic, restated here.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine import YolopError, load_library

BN_EPS = 1e-3
INPUT_IMG_SIZE = 380
NUM_CLASSES = 2
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
THRESHOLDS = (0.9, 0.8, 0.7, 0.6)

# efficientnet_pytorch 0.7.x: efficientnet-b0 block strings (repeats, kernel, stride, expand, in, out), se_ratio 0.25
_B0 = [(1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80),
       (3, 5, 1, 6, 80, 112), (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320)]
# efficientnet_params(): (width, depth, image size, dropout); only b3 is built - b4/b5/b7 are registered by the reference, never used
_PARAMS = {"efficientnet-b3": (1.2, 1.4, 300, 0.3)}
_UNUSED = ("efficientnet-b4", "efficientnet-b5", "efficientnet-b7")


def round_filters(filters: int, width: float, divisor: int = 8) -> int:
    x = filters * width
    nf = max(divisor, int(x + divisor / 2) // divisor * divisor)
    if nf < 0.9 * x:
        nf += divisor
    return int(nf)


def same_padding(size: int, k: int, s: int) -> Tuple[int, int]:
    """Conv2dStaticSamePadding for an input of `size`: (before, after)."""
    total = max((math.ceil(size / s) - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def _check_name(name: str) -> Tuple[float, float, int]:
    if name in _UNUSED:
        raise ValueError(f"{name} is registered by the reference but never selected; only efficientnet-b3 is built")
    if name not in _PARAMS:
        raise ValueError(f"unknown network {name!r} (efficientnet-b3)")
    w, d, img, _ = _PARAMS[name]
    return w, d, img


def block_specs(name: str = "efficientnet-b3") -> List[dict]:
    """One dict per MBConv block: stage, k, s, cin, cout, cexp, sq, expand, residual, pad (the depthwise conv's static pad for the
    configured image size), hin/hout (map sizes for the 380x380 input)."""
    width, depth, img = _check_name(name)
    out = []
    isz, h = math.ceil(img / 2), math.ceil(INPUT_IMG_SIZE / 2)
    for si, (r, k, s, e, i, o) in enumerate(_B0):
        cin0, cout = round_filters(i, width), round_filters(o, width)
        for j in range(int(math.ceil(depth * r))):
            st = s if j == 0 else 1
            cin = cin0 if j == 0 else cout
            out.append(dict(stage=si + 1, k=k, s=st, cin=cin, cout=cout, cexp=cin * e, sq=max(1, int(cin * 0.25)), expand=e != 1,
                            residual=st == 1 and cin == cout, pad=same_padding(isz, k, st), hin=h, hout=math.ceil(h / st)))
            isz, h = math.ceil(isz / st), math.ceil(h / st)
    return out


def padding_table(name: str = "efficientnet-b3") -> Dict[str, Tuple[int, int]]:
    """Static (before, after) padding of every spatial conv (1x1 convs have none): '_conv_stem' and '_blocks.{i}._depthwise_conv'."""
    _, _, img = _check_name(name)
    t = {"_conv_stem": same_padding(img, 3, 2)}
    for i, b in enumerate(block_specs(name)):
        t[f"_blocks.{i}._depthwise_conv"] = b["pad"]
    return t


def head_width(name: str = "efficientnet-b3") -> int:
    return round_filters(1280, _check_name(name)[0])


def state_shapes(name: str = "efficientnet-b3", num_classes: int = NUM_CLASSES) -> Dict[str, Tuple[int, ...]]:
    """Every key of the efficientnet_pytorch state dict with its shape (BatchNorm: weight, bias, running_mean, running_var,
    num_batches_tracked)."""
    width = _check_name(name)[0]
    sh: Dict[str, Tuple[int, ...]] = {}

    def bn(p, c):
        for s in ("weight", "bias", "running_mean", "running_var"):
            sh[f"{p}.{s}"] = (c,)
        sh[f"{p}.num_batches_tracked"] = ()

    c0 = round_filters(32, width)
    sh["_conv_stem.weight"] = (c0, 3, 3, 3)
    bn("_bn0", c0)
    blocks = block_specs(name)
    for i, b in enumerate(blocks):
        p = f"_blocks.{i}"
        if b["expand"]:
            sh[f"{p}._expand_conv.weight"] = (b["cexp"], b["cin"], 1, 1)
            bn(f"{p}._bn0", b["cexp"])
        sh[f"{p}._depthwise_conv.weight"] = (b["cexp"], 1, b["k"], b["k"])
        bn(f"{p}._bn1", b["cexp"])
        sh[f"{p}._se_reduce.weight"] = (b["sq"], b["cexp"], 1, 1)
        sh[f"{p}._se_reduce.bias"] = (b["sq"],)
        sh[f"{p}._se_expand.weight"] = (b["cexp"], b["sq"], 1, 1)
        sh[f"{p}._se_expand.bias"] = (b["cexp"],)
        sh[f"{p}._project_conv.weight"] = (b["cout"], b["cexp"], 1, 1)
        bn(f"{p}._bn2", b["cout"])
    hc = head_width(name)
    sh["_conv_head.weight"] = (hc, blocks[-1]["cout"], 1, 1)
    bn("_bn1", hc)
    sh["_fc.weight"] = (num_classes, hc)
    sh["_fc.bias"] = (num_classes,)
    return sh


def param_count(name: str = "efficientnet-b3") -> int:
    """Trainable parameters (BatchNorm running statistics excluded), as model.parameters() counts them."""
    return sum(int(np.prod(s)) for k, s in state_shapes(name).items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))


GAINS = {"bn": 1.0, "conv": 3.0, "_depthwise_conv": 3.0, "_se_reduce": 2.0, "_se_expand": 2.0, "_project_conv": 0.35, "_fc": 32.0}


def synthetic_state(seed: int = 0, name: str = "efficientnet-b3") -> Dict[str, torch.Tensor]:
    """Seeded state dict in efficientnet_pytorch's layout (no checkpoint exists offline). BatchNorm statistics sit away from the identity
    so that the fold is exercised; the gains keep the activations O(1) through the 26 blocks (the residual stream does not blow up) and
    leave the two logits a few units apart (neither tied nor saturated)."""
    g = torch.Generator().manual_seed(seed)
    st: Dict[str, torch.Tensor] = {}
    for k, shape in state_shapes(name).items():
        if k.endswith("num_batches_tracked"):
            st[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_mean"):
            st[k] = torch.randn(shape, generator=g) * 0.1
        elif k.endswith("running_var"):
            st[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith(".bias"):
            is_bn = k.rsplit(".", 1)[0].split(".")[-1].startswith("_bn")
            st[k] = (torch.rand(shape, generator=g) - 0.5) * (0.1 if is_bn else 0.2)
        elif len(shape) == 1:      # BN gamma
            st[k] = GAINS["bn"] * (0.6 + 0.8 * torch.rand(shape, generator=g))
        else:
            fan = int(np.prod(shape[1:]))
            gain = GAINS.get(k.split(".")[-2], GAINS["conv"])
            st[k] = torch.randn(shape, generator=g) * (gain / fan) ** 0.5
    return st


def fold_state(state: Dict[str, torch.Tensor], name: str = "efficientnet-b3") -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """Conv + eval-mode BatchNorm -> one (weight, bias) per module (fp64 fold, fp32 out), keyed by the conv's module name; the SE convs
    and the FC layer pass through."""
    def fold(conv, bn):
        w = state[f"{conv}.weight"].double()
        s = state[f"{bn}.weight"].double() / torch.sqrt(state[f"{bn}.running_var"].double() + BN_EPS)
        b = state[f"{bn}.bias"].double() - state[f"{bn}.running_mean"].double() * s
        return (w * s.view(-1, *([1] * (w.dim() - 1)))).float(), b.float()

    out = {"_conv_stem": fold("_conv_stem", "_bn0")}
    for i, b in enumerate(block_specs(name)):
        p = f"_blocks.{i}"
        if b["expand"]:
            out[f"{p}._expand_conv"] = fold(f"{p}._expand_conv", f"{p}._bn0")
        out[f"{p}._depthwise_conv"] = fold(f"{p}._depthwise_conv", f"{p}._bn1")
        for m in ("_se_reduce", "_se_expand"):
            out[f"{p}.{m}"] = (state[f"{p}.{m}.weight"].float(), state[f"{p}.{m}.bias"].float())
        out[f"{p}._project_conv"] = fold(f"{p}._project_conv", f"{p}._bn2")
    out["_conv_head"] = fold("_conv_head", "_bn1")
    out["_fc"] = (state["_fc.weight"].float(), state["_fc.bias"].float())
    return out


# ---- checkpoints (what timm's load_checkpoint(model, path) accepts, strict) -------------------------------------------------------------
def read_checkpoint(path: str, name: str = "efficientnet-b3") -> Dict[str, torch.Tensor]:
    """A raw state dict, or a dict holding one under 'state_dict_ema' (preferred, as timm's use_ema default) or 'state_dict'; keys may
    carry a 'module.' prefix. Raises KeyError / ValueError naming the first missing, unexpected or mis-shaped key."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such checkpoint (nothing is downloaded)")
    try:
        ck = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:
        # timm training checkpoints (.pth.tar) pickle their argparse namespace next to the weights; timm unpickles them in full too
        ck = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(ck, dict):
        for key in ("state_dict_ema", "state_dict"):
            if isinstance(ck.get(key), dict):
                ck = ck[key]
                break
    if not isinstance(ck, dict):
        raise ValueError(f"{path}: not a state dict")
    state = {(k[7:] if k.startswith("module.") else k): v for k, v in ck.items()}
    check_state(state, name)
    return state


def check_state(state: Dict[str, torch.Tensor], name: str = "efficientnet-b3") -> None:
    want = state_shapes(name)
    for k, s in want.items():
        if k not in state:
            raise KeyError(f"missing key {k!r} in the classifier state dict")
        if tuple(state[k].shape) != s:
            raise ValueError(f"key {k!r}: shape {tuple(state[k].shape)}, expected {s}")
    for k in state:
        if k not in want:
            raise KeyError(f"unexpected key {k!r} in the classifier state dict")


# ---- the engine --------------------------------------------------------------------------------------------------------------------------
def _declare(lib: C.CDLL) -> None:
    if getattr(lib, "_cls_declared", False):
        return
    vp = C.c_void_p
    lib.yp_cls_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    lib.yp_cls_destroy.argtypes = [vp]
    lib.yp_cls_weight_count.argtypes = [vp]
    lib.yp_cls_weight_info.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    lib.yp_cls_set_weight.argtypes = [vp, C.c_char_p, vp, C.POINTER(C.c_int64), C.c_int]
    lib.yp_cls_finalize.argtypes = [vp]
    lib.yp_cls_forward.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.yp_cls_set_graph.argtypes = [vp, C.c_int]
    lib.yp_cls_tensor_count.argtypes = [vp]
    lib.yp_cls_tensor_info.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    lib.yp_cls_tensor_read.argtypes = [vp, C.c_int, vp]
    for fn in ("yp_cls_create", "yp_cls_destroy", "yp_cls_weight_count", "yp_cls_weight_info", "yp_cls_set_weight", "yp_cls_finalize",
               "yp_cls_forward", "yp_cls_set_graph", "yp_cls_tensor_count", "yp_cls_tensor_info", "yp_cls_tensor_read"):
        getattr(lib, fn).restype = C.c_int
    lib._cls_declared = True


class ClassifierEngine:
    """One engine per GPU. dtype 'fp32' (default: the reference runs in fp32 and its 0.6-0.9 thresholds decide the insertion frame) =
    exact fp32 FMA chains; 'bf16' = bf16 storage with fp32 accumulation (SE, pooling and softmax stay fp32)."""

    def __init__(self, dtype: str = "fp32", device: int = 0, state: Optional[Dict[str, torch.Tensor]] = None, name: str = "efficientnet-b3"):
        _check_name(name)
        self.lib = load_library()
        _declare(self.lib)
        self.name, self.dtype, self.device_index = name, dtype, int(device)
        self._h = C.c_void_p()
        self._chk(self.lib.yp_cls_create(int(name[-1]), {"bf16": 0, "fp32": 1, "f32": 1}[dtype], self.device_index, C.byref(self._h)))
        if state is not None:
            self.load_state(state)
            self.finalize()

    def _chk(self, rc: int) -> int:
        if rc < 0:
            raise YolopError(f"libyolop error {rc}: {self.lib.yp_last_error().decode()}")
        return rc

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.yp_cls_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def expected_weights(self) -> List[Tuple[str, Tuple[int, ...]]]:
        n = self._chk(self.lib.yp_cls_weight_count(self._h))
        name = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        out = []
        for i in range(n):
            self._chk(self.lib.yp_cls_weight_info(self._h, i, name, 256, shape, C.byref(nd)))
            out.append((name.value.decode(), tuple(int(shape[j]) for j in range(nd.value))))
        return out

    def load_state(self, state: Dict[str, torch.Tensor]) -> None:
        check_state(state, self.name)
        for mod, (w, b) in fold_state(state, self.name).items():
            for suffix, t in ((".weight", w), (".bias", b)):
                t = t.detach().to(torch.float32).contiguous().cpu()
                shp = (C.c_int64 * t.dim())(*t.shape)
                self._chk(self.lib.yp_cls_set_weight(self._h, (mod + suffix).encode(), C.c_void_p(t.data_ptr()), shp, t.dim()))

    def finalize(self) -> None:
        self._chk(self.lib.yp_cls_finalize(self._h))

    def set_graph(self, enable: bool) -> None:
        self._chk(self.lib.yp_cls_set_graph(self._h, 1 if enable else 0))

    def forward(self, frames: torch.Tensor, boxes: torch.Tensor, bgr: bool = True):
        """frames uint8 cuda [B,H,W,3], boxes int32 cuda [B,4] xyxy -> (logits float32 [B,2], max prob float32 [B], class int32 [B])."""
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3):
            raise TypeError("forward expects uint8 CUDA frames [B,H,W,3]")
        B, H, W, _ = frames.shape
        if not (boxes.is_cuda and boxes.dtype == torch.int32 and tuple(boxes.shape) == (B, 4)):
            raise TypeError("forward expects int32 CUDA boxes [B,4]")
        frames, boxes = frames.contiguous(), boxes.contiguous()
        dev = frames.device
        logits = torch.empty((B, 2), dtype=torch.float32, device=dev)
        prob = torch.empty((B,), dtype=torch.float32, device=dev)
        cls = torch.empty((B,), dtype=torch.int32, device=dev)
        self._chk(self.lib.yp_cls_forward(self._h, C.c_void_p(frames.data_ptr()), B, H, W, 1 if bgr else 0, C.c_void_p(boxes.data_ptr()),
                                          C.c_void_p(logits.data_ptr()), C.c_void_p(prob.data_ptr()), C.c_void_p(cls.data_ptr()),
                                          C.c_void_p(int(torch.cuda.current_stream(dev).cuda_stream))))
        self._last = (frames, boxes)
        return logits, prob, cls

    def tensors(self) -> List[dict]:
        n = self._chk(self.lib.yp_cls_tensor_count(self._h))
        name = C.create_string_buffer(256)
        dims = (C.c_int * 4)()
        return [dict(index=i, name=(self._chk(self.lib.yp_cls_tensor_info(self._h, i, name, 256, dims)), name.value.decode())[1], shape=tuple(dims))
                for i in range(n)]

    def read_tensor(self, name: str) -> torch.Tensor:
        """Debug tap: NHWC fp32 host copy of an activation of the last forward ('input', 'stem', '_blocks.{i}.expand' / '.dw' / '.gate',
        '_blocks.{i}' = block output, 'head.pool')."""
        for t in self.tensors():
            if t["name"] == name:
                out = torch.empty(t["shape"], dtype=torch.float32)
                self._chk(self.lib.yp_cls_tensor_read(self._h, t["index"], C.c_void_p(out.data_ptr())))
                return out
        raise KeyError(name)


# ---- host restatement of the reference's crop, search and repair -------------------------------------------------------------------------
def crop_geometry(box: Sequence[int], height: int, width: int, crop_size: int = INPUT_IMG_SIZE) -> Tuple[int, int, int, int]:
    """crop_frame's window for an integer xyxy box: (x0, y0, cw, ch) - the clipped window starts at (x0, y0) and is cw x ch; it lands at
    the top-left of the zero crop_size^2 image whenever it is short of crop_size (need_padding=True). The same
    integer arithmetic runs on the device (effnet.hip roi_of)."""
    x1, y1, x2, y2 = (int(v) for v in box)
    cx, cy = int((x1 + x2) / 2), int((y1 + y2) / 2)
    half = crop_size // 2
    wx1, wy1 = max(0, cx - half), max(0, cy - half)
    wx2, wy2 = min(width, cx + half), min(height, cy + half)
    return wx1, wy1, max(0, wx2 - wx1), max(0, wy2 - wy1)


def crop_roi(frame: np.ndarray, box: Sequence[int], crop_size: int = INPUT_IMG_SIZE) -> np.ndarray:
    """The uint8 crop_size^2 image crop_frame(frame, box, crop_size, need_padding=True) returns."""
    h, w = frame.shape[:2]
    x0, y0, cw, ch = crop_geometry(box, h, w, crop_size)
    out = np.zeros((crop_size, crop_size, 3), dtype=np.uint8)
    out[:ch, :cw] = frame[y0:y0 + ch, x0:x0 + cw]
    return out


def find_insert_index(class_list: Sequence[int], prob_list: Sequence[float], judge_wnd: int = 20) -> int:
    """The insertion frame: scan the windows of judge_wnd frames in order; in a window with at least 0.9 judge_wnd class-1 frames, try the
    thresholds 0.9 .. 0.6 in order for the first offset k <= judge_wnd - 5 that starts five class-1 frames with prob > threshold; the
    first hit is window start + k. A qualifying window without a hit does not end the scan. No hit at all (or fewer than judge_wnd
    frames): 0."""
    n = len(class_list)
    need = 0.9 * judge_wnd
    for i in range(n - judge_wnd + 1):
        cls = class_list[i:i + judge_wnd]
        if sum(1 for c in cls if c == 1) < need:
            continue
        prb = prob_list[i:i + judge_wnd]
        for t in THRESHOLDS:
            for k in range(judge_wnd - 4):
                if all(cls[k + l] == 1 and prb[k + l] > t for l in range(5)):
                    return i + k
    return 0


def fix_class_prob(class_list: list, prob_list: list, class_index: int):
    """Repair in place: before class_index every frame becomes class 0 (prob of the nearest earlier class-0 frame, else 0.6); after it
    every frame becomes class 1 (prob of the nearest later class-1 frame, else 0.6). The searches look at entries not yet rewritten."""
    n = len(class_list)
    for i in range(class_index - 1, -1, -1):
        if class_list[i] != 0:
            p = next((prob_list[j] for j in range(i - 1, -1, -1) if class_list[j] == 0), 0.6)
            class_list[i], prob_list[i] = 0, p
    for i in range(class_index + 1, n):
        if class_list[i] != 1:
            p = next((prob_list[j] for j in range(i + 1, n) if class_list[j] == 1), 0.6)
            class_list[i], prob_list[i] = 1, p
    return class_list, prob_list


# ---- the reference's entry points (yolo_seg/tasks/needle_clasify.py) --------------------------------------------------------------------
def _device_index(device) -> int:
    d = torch.device(device if device != "cuda" else "cuda:0")
    if d.type != "cuda":
        raise ValueError("this engine runs on MI355X GPUs only")
    return d.index or 0


def _load_net(model_name: str, num_classes: int = NUM_CLASSES, checkpoint: Optional[str] = None, device="cuda", dtype: str = "fp32"):
    if model_name.startswith("van"):
        raise NotImplementedError(f"{model_name}: the VAN classifiers are registered by the reference but never selected; not ported")
    if num_classes != NUM_CLASSES:
        raise ValueError(f"num_classes={num_classes!r}: the needle classifier has {NUM_CLASSES} classes")
    name = model_name.replace("_", "-")
    _check_name(name)
    if not checkpoint:
        raise ValueError("a checkpoint is required (pretrained weights are not downloaded)")
    return ClassifierEngine(dtype, _device_index(device), state=read_checkpoint(checkpoint, name), name=name)


def load_classify_net(checkpoint_name: Optional[str] = None, device="cuda", *, name: Optional[str] = None, weights_dir: Optional[str] = None,
                      dtype: str = "fp32") -> ClassifierEngine:
    """`load_classify_net(checkpoint_name, device)` and the app's `load_classify_net(name=...)` (SURVEY C-1): loads the efficientnet_b3
    checkpoint `weights_dir/checkpoint_name` (an absolute or existing path is taken as is). Fixes C-2: the path is the checkpoint."""
    ck = name if name is not None else checkpoint_name
    if ck is None:
        raise TypeError("load_classify_net needs a checkpoint name")
    path = ck if (os.path.isabs(ck) or os.path.isfile(ck)) else os.path.join(weights_dir or os.environ.get("YOLOP_WEIGHTS_PATH", "weights"), ck)
    return _load_net("efficientnet_b3", NUM_CLASSES, checkpoint=path, device=device, dtype=dtype)


def _resize_380(image: np.ndarray) -> np.ndarray:
    if image.shape[0] == INPUT_IMG_SIZE and image.shape[1] == INPUT_IMG_SIZE:
        return image                                              # PIL returns a copy at equal size: identity
    from PIL import Image
    return np.asarray(Image.fromarray(image).resize((INPUT_IMG_SIZE, INPUT_IMG_SIZE), Image.BILINEAR))


def predict_images(model: ClassifierEngine, images):
    """RGB uint8 HWC images -> (indices, probabilities): lists of numpy scalars (int64 class, float32 max softmax), as the reference."""
    if len(images) == 0:
        return [], []
    batch = np.stack([np.ascontiguousarray(_resize_380(np.asarray(im, dtype=np.uint8))) for im in images])
    dev = torch.device("cuda", model.device_index)
    x = torch.from_numpy(batch).to(dev)
    boxes = torch.tensor([[0, 0, INPUT_IMG_SIZE, INPUT_IMG_SIZE]] * len(images), dtype=torch.int32, device=dev)
    _, prob, cls = model.forward(x, boxes, bgr=False)
    return list(cls.cpu().numpy().astype(np.int64)), list(prob.cpu().numpy())


def predict_and_find_start_inserted(model: ClassifierEngine, frames=None, boxes_list=None, judge_wnd: int = 20, batch_size: int = 8):
    """BGR frames + integer xyxy boxes -> (class_list, prob_list, insert_frame_index), repaired. frames: BGR uint8 HWC ndarrays, which go
    up in chunks of batch_size, or a uint8 CUDA tensor [N,H,W,3] on the model's device (a clip uploaded once), sliced per chunk. Frames
    are cropped on the device; every image's result is independent of the chunking."""
    frames = [] if frames is None else frames
    boxes_list = [] if boxes_list is None else boxes_list
    dev = torch.device("cuda", model.device_index)
    on_dev = isinstance(frames, torch.Tensor)
    if on_dev:
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3):
            raise TypeError("predict_and_find_start_inserted expects BGR uint8 HWC ndarrays or a uint8 CUDA tensor [N,H,W,3]")
        if frames.device != dev:
            raise ValueError(f"frames are on {frames.device}, the model on {dev}")
        frames = frames.contiguous()
    if len(frames) != len(boxes_list):
        raise ValueError("The length of frames and boxes_list must be the same.")
    class_list: list = []
    prob_list: list = []
    for i in range(0, len(frames), batch_size):
        chunk = frames[i:i + batch_size]
        if on_dev:
            x = chunk
        else:
            x = torch.from_numpy(np.stack([np.ascontiguousarray(f, dtype=np.uint8) for f in chunk])).to(dev)
        b = torch.tensor([[int(v) for v in bx] for bx in boxes_list[i:i + batch_size]], dtype=torch.int32, device=dev)
        _, prob, cls = model.forward(x, b, bgr=True)
        class_list.extend(cls.cpu().numpy().astype(np.int64))
        prob_list.extend(prob.cpu().numpy())
    idx = find_insert_index(class_list, prob_list, judge_wnd)
    fix_class_prob(class_list, prob_list, idx)
    return class_list, prob_list, idx
