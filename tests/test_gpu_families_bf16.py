"""YOLOv8-seg / YOLO11-seg in bf16 (the dtype `YOLO(...)` loads these checkpoints with), one op at a time: the teacher-forced per-op contract
of the YOLOv10 graphs (perop_bf16.py) on the C2f / C3k2 / C3k / C2PSA trunks and the Segment head - 16 / 32 / 48 /
96-channel 3x3 layers, the v8 head's dense 3x3 class convs (80 wide), conv_igemm_kernel in bf16 (11-n / 11-s), the cls_out pass and the
class branch's conv_dwpw TAIL form - and every conv tile configuration id on a family graph that takes it."""
import pytest

from perop_bf16 import FAMILY_SWEEP, per_op_bf16

pytestmark = pytest.mark.gpu

SHAPES = {"n": (2, 96, 128), "s": (1, 160, 192), "m": (1, 64, 96), "l": (1, 64, 64), "x": (1, 64, 64)}     # the fp32 layerwise shapes
# where the plan's cls_out pass applies at nc = 80 (class logits + class-max keys in one launch, one per level): a 64..512-wide, K % 64 == 0
# input to the logit conv that fits the kernel's LDS (v8-n / 11-n: 80- / 64-wide rows of a 16-channel-per-lane kernel are not; 11-x: LDS)
CLS_OUT = {("v8", "s"), ("v8", "m"), ("v8", "l"), ("v8", "x"), ("11", "s"), ("11", "m"), ("11", "l")}


def _check(family, variant, shape, monkeypatch, cfg=-1, fuse=True, nc=80, autotune=False, want_tail=False):
    r = per_op_bf16(variant, True, shape, cfg, fuse, monkeypatch, nc, want_tail=want_tail, family=family, autotune=autotune)
    if fuse and nc == 80 and not want_tail:
        assert r["nclsout"] == (3 if (family, variant) in CLS_OUT else 0), r
    return r


@pytest.mark.parametrize("family,variant,shape", [(f, v, SHAPES[v]) for f in ("11", "v8") for v in "nsmlx"] +
                         [("11", "s", (1, 480, 608)), ("v8", "s", (1, 480, 608))])      # 60x76 at P3: partial tiles of every tiled kernel
def test_per_op_bf16_heuristic(family, variant, shape, monkeypatch):
    """The heuristic's tile configurations (autotune off: a function of the build and the shape only)."""
    r = _check(family, variant, shape, monkeypatch)
    assert r["nfused"] + r["npwsp"] > 0


@pytest.mark.parametrize("family", ["11", "v8"])
def test_per_op_bf16_autotuned(family, monkeypatch):
    """The tuner's configurations for this box (what a first forward of a new shape runs with)."""
    _check(family, "s", SHAPES["s"], monkeypatch, autotune=True)


@pytest.mark.parametrize("family,variant,nc", [("11", "n", 1), ("v8", "n", 3), ("11", "s", 3), ("v8", "s", 1)])
def test_per_op_bf16_small_nc(family, variant, nc, monkeypatch):
    """The needle fine-tunes' class counts: 1- / 3-channel fp32 class maps, the class branch at max(c3, min(nc, 100)) width."""
    _check(family, variant, SHAPES[variant], monkeypatch, nc=nc)


@pytest.mark.parametrize("family", ["11", "v8"])
def test_per_op_bf16_unfused(family, monkeypatch):
    """YOLOP_NO_FUSE=1: every fused pair's stages as stand-alone kernels, under the strict per-op bound."""
    _check(family, "s", SHAPES["s"], monkeypatch, fuse=False)


def test_per_op_bf16_tail_form(monkeypatch):
    """YOLOP_TAIL=1 on 11-s at nc = 80: YOLO11's class branch (dw -> pw -> dw -> pw -> logits) with the logit conv and the class-max keys as
    the third stage of conv_dwpw - the 128-wide branch on the 32x40 / 16x20 maps (the 8x10 level stays a cls_out launch)."""
    monkeypatch.setenv("YOLOP_TAIL", "1")
    r = _check("11", "s", (1, 256, 320), monkeypatch, want_tail=True)
    assert r["ntail"] > 0 and r["nclsout"] > 0


@pytest.mark.parametrize("family,variant,seg,shape,cfg,fuse", FAMILY_SWEEP)
def test_per_op_bf16_forced_cfg(family, variant, seg, shape, cfg, fuse, monkeypatch):
    """Every conv tile configuration id, forced wherever it is valid, on a family graph where ops take it."""
    r = _check(family, variant, shape, monkeypatch, cfg=cfg, fuse=fuse)
    assert r["ntaken"] > 0
