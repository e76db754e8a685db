"""16-byte conv stores in the paired channel order (csrc/kernel_util.h) against the 8-byte form: bit for bit.

Two engines are built from one seeded state, one of them under YOLOP_NARROW_STORE=1 (read at yp_create: it keeps the 8-byte stores
everywhere). Every tensor of the narrow engine is then overwritten with the wide engine's, so both step an op from identical inputs AND
identical surroundings of its output slice. An op is stepped in both with yp_run_op and the WHOLE output tensor is compared with
torch.equal - a store that strays into a neighbouring concat slice fails as well. The paired order changes no arithmetic (the same dot
product in the same k order per output element), so nothing but equality is admissible.

yp_debug_last_store_form reports, host-side, which form the last launch took: the cases assert that the wide engine really launched the
16-byte form where the family has it, that the narrow engine never did, and that the fallback (odd fragment count per wave, misaligned or
narrow slices) was exercised and agrees too."""
import os

import pytest
import torch

from helpers import make_case
from perop_bf16 import V10_SWEEP

pytestmark = pytest.mark.gpu

# one sweep case per configuration id of the families whose kernels have the paired form (shapes at which the id is taken, partial tiles
# included: 12x20, 24x40 and 6x10 maps do not divide by the 8x16 / 16x16 tiles)
_S_SEG = {c[4]: c for c in V10_SWEEP if c[0] == "v10" and c[1] == "s" and c[2] and c[5]}
TILE1_IDS = (600, 601)                       # conv_tile1 <4>, <2> (conv_tile1w, id 602, measured no gain and has the 8-byte form only)
WREG_IDS = (703, 704, 705, 706, 708, 712)    # conv_wreg: 4 and 2 channel fragments per wave, 16- and 8-wide tiles, one and two waves per SIMD
PXD_IDS = (800, 802, 805, 807)               # conv_pxd (1x1): 16, 8 and 4 channel fragments per wave, one and two waves in N
WREG_ODD_IDS = (709, 710, 700, 702)          # conv_wreg with ONE channel fragment per wave (no pair to store) or 16 accumulator fragments (no
                                             # registers for two epilogues: conv_wreg.hip, wreg_paired): always the 8-byte form

_PAIRS = {}


def _create(variant, seg, st, **env):
    from yolo_puncture_amd.engine import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                     # (switches read at yp_create)
    try:
        return Engine(variant, 80, seg, "bf16", 0, state={k: v.clone() for k, v in st.items()})
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _pair(variant, seg, shape, fuse=True):
    """(wide engine, narrow engine, frames, outputs of both forwards), tensors of both set to the wide one's. fuse=False: every op runs as
    its own kernel (YOLOP_NO_FUSE=1), so the 1x1 convs that the fused forms swallow are launched - and stepped - as plain convs."""
    key = (variant, seg, tuple(shape), fuse)
    if key not in _PAIRS:
        for k in list(_PAIRS):                # one pair alive at a time
            for e in _PAIRS.pop(k)[:2]:
                e.close()
        st, im = make_case(variant, 80, seg, 0, shape)
        imc = im.cuda()
        nofuse = {} if fuse else {"YOLOP_NO_FUSE": "1"}
        wide = _create(variant, seg, st, **nofuse)
        narrow = _create(variant, seg, st, YOLOP_NARROW_STORE="1", **nofuse)
        outs = []
        for e in (wide, narrow):
            e.set_autotune(False)
            outs.append(e.forward(imc))
        torch.cuda.synchronize()
        for t in wide.tensors():                  # (memory no op of the forward wrote may hold NaN patterns: not comparable, so cleared)
            if all(d > 0 for d in t["shape"]):
                v = torch.nan_to_num(wide.read_tensor(t["index"]), nan=0.0, posinf=0.0, neginf=0.0)
                wide.write_tensor(t["index"], 0, v)
                narrow.write_tensor(t["index"], 0, v)
        _PAIRS[key] = (wide, narrow, imc, outs)
    return _PAIRS[key]


def _step_both(pair, shape, cfg, want=None):
    """Step every op that launches with the forced id `cfg` (or the ops named in `want`, under it) in both engines; -> {op: (store form of
    the wide engine's launch, output tensor is fp32)}. The narrow engine's launches must all report the 8-byte form."""
    from yolo_puncture_amd.engine import load_library
    lib = load_library()
    wide, narrow, imc, outs = pair
    lib.yp_debug_force_conv_cfg(cfg)
    try:
        ops = wide.plan(*shape)
        ops_n = narrow.plan(*shape)
        assert [(o["name"], o["kernel"], o["cfg"]) for o in ops] == [(o["name"], o["kernel"], o["cfg"]) for o in ops_n]   # no configuration id, no symbol depends on the switch
        forms = {}
        f32 = {t["index"]: t["f32"] for t in wide.tensors()}
        for i, o in enumerate(ops):
            if o["kind"] == "head" or (want is None and o["cfg"] != cfg) or (want is not None and o["name"] not in want):
                continue
            lib.yp_debug_last_store_form()         # (reading resets it: -1 below = the op's kernel has one form only)
            wide.run_op(i, imc, outs[0])
            fw = lib.yp_debug_last_store_form()
            narrow.run_op(i, imc, outs[1])
            fn = lib.yp_debug_last_store_form()
            torch.cuda.synchronize()
            t = o["out"][0]
            a, b = wide.read_tensor(t), narrow.read_tensor(t)
            print(f"  cfg {cfg} {o['name']:28s} {o['kernel'][:44]:44s} out {o['out']} store form wide engine {fw} narrow engine {fn} "
                  f"differing elements {int((a != b).sum())}")
            assert fn <= 0, (o["name"], "the narrow engine launched the 16-byte form")
            assert torch.equal(a, b), (cfg, o["name"], o["kernel"])
            forms[o["name"]] = (fw, f32[t])
        return forms
    finally:
        lib.yp_debug_force_conv_cfg(-1)


@pytest.mark.parametrize("cfg", sorted(TILE1_IDS + WREG_IDS + PXD_IDS, key=lambda c: (_S_SEG[c][3], c)))    # (cases of one shape share an engine pair)
def test_paired_family_ids(cfg):
    _, variant, seg, shape, c, _ = _S_SEG[cfg]
    forms = _step_both(_pair(variant, seg, shape), shape, c)
    assert forms, f"no op took configuration {cfg}"
    # v10-S: every slice is 32-channel aligned, so every such layer is paired.
    # The head's last 1x1s write fp32 logits: those already store 16 bytes per lane and have no paired form.
    assert any(f == 1 for f, _ in forms.values()), forms
    assert all(f == 0 for f, is32 in forms.values() if is32), forms
    assert all(f == 1 for f, is32 in forms.values() if not is32), forms


@pytest.mark.parametrize("cfg", WREG_ODD_IDS)
def test_one_fragment_per_wave_falls_back(cfg):
    _, variant, seg, shape, c, _ = _S_SEG[cfg]
    forms = _step_both(_pair(variant, seg, shape), shape, c)
    assert forms and all(f == 0 for f, _ in forms.values()), forms


def test_residual_concat_slice_and_folded_upsample():
    """model.4.m.0.cv2 adds a residual; model.4.cv1 / model.13.cv1 write into concat buffers that other ops fill beside them (model.13.cv1's
    slice starts at a non-zero channel); model.16.cv1 reads the folded nearest-x2 upsample. Each under the plan's own pick and under the 3x3
    ids (which the 3x3 residual layer takes; the 1x1 layers keep their kernels)."""
    shape = (1, 256, 256)
    pair = _pair("s", True, shape)
    names = ("model.4.m.0.cv2", "model.4.cv1", "model.13.cv1", "model.16.cv1")
    seen = {}
    for cfg in (-1, 600, 706, 708):
        for n, (f, _) in _step_both(pair, shape, cfg, want=names).items():
            seen.setdefault(n, set()).add(f)
    assert set(seen) == set(names), seen
    assert 1 in seen["model.4.m.0.cv2"], seen             # the residual layer ran paired (16-byte residual reads) at least once


def test_v10n_alignment_fallback():
    """v10-N, every op as its own kernel: the class branch's 80-channel 1x1 convs (not whole 32-channel fragment pairs) and the 16- / 48-channel
    layers miss the conditions of the paired form. Both engines agree on every op under the plan's own picks and under every id of the paired
    families, and the fallback is OBSERVED, not assumed."""
    shape = (2, 96, 128)
    pair = _pair("n", True, shape, fuse=False)
    forms = []
    wide = pair[0]
    names = [o["name"] for o in wide.plan(*shape) if o["kind"] != "head"]
    forms += list(_step_both(pair, shape, -1, want=names).values())
    for cfg in TILE1_IDS + WREG_IDS + WREG_ODD_IDS + PXD_IDS:
        lib_forms = _step_both(pair, shape, cfg)
        forms += list(lib_forms.values())
    print("v10-N (store form, fp32 output) seen:", {f: forms.count(f) for f in set(forms)})
    assert (0, False) in forms, "no bf16 launch of v10-N took the 8-byte fallback"
    assert (1, False) in forms, "no launch of v10-N took the 16-byte form"


def test_chained_forward_equal():
    """the whole forward: det / idx of the two engines equal bit for bit"""
    shape = (2, 256, 384)
    wide, narrow, imc, _ = _pair("s", True, shape)
    a, b = wide.forward(imc), narrow.forward(imc)
    torch.cuda.synchronize()
    for k in ("det", "idx"):
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    for e in _PAIRS.pop(("s", True, shape, True))[:2]:
        e.close()
