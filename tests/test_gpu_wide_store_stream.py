"""16-byte stores in the paired channel order for the streaming and fused conv kernels that gained from them: conv_wres<128,2> (id 1101),
conv_dwpw_stream<4>, c2f_fused and the plain form of pwsp - bit for bit against the 8-byte form; and the kernels of those families that keep
the 8-byte form (conv_wres ids 1100 / 1102, conv_dwpw_stream<8>, pwsp's spatial forms), observed to take it and to agree.

The method is tests/test_gpu_wide_store.py's (its engine-pair cache is shared, so one pair is alive at a time across both files): two engines
from one seeded state, one under YOLOP_NARROW_STORE=1, every tensor of the narrow engine overwritten with the wide engine's; an op is stepped in
both with yp_run_op and the WHOLE output tensor compared with torch.equal (a store that strays into a neighbouring concat slice fails too).
yp_debug_last_store_form says which form a launch took: the wide engine must have taken the 16-byte form wherever the launcher's conditions
hold (restated here from the layer's width), the narrow engine never, and every fallback is observed.

What can go silently wrong in these kernels is the COUNTED wait in front of a tile (`vmcnt(<stores issued behind the tile's rows>)`): the
paired form issues half the stores, and with the narrow count the MFMAs would read rows that have not landed. That wait only matters from a
workgroup's second tile on, so every case runs a second time under yp_debug_max_workgroups(3): a workgroup then walks several tiles
(asserted from the tile count). Every launch runs twice and both results must be equal - a race that merely got lucky once would differ.

Not reachable on v10-S, so not here: model.13.cv1 as conv_wres (its 768-channel rows do not fit beside two pixel tiles in LDS under any of the
three ids; the folded-upsample form runs through model.16.cv1 under 1102, the non-zero channel offset through model.4.cv2 and model.13.cv2).
frontend_kernel and conv_halo_s2 keep the 8-byte form alone and have no case."""
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":                                 # (the child of test_conv_dwpw_stream_one_workgroup_per_cu_is_narrow)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from test_gpu_wide_store import _pair, _PAIRS

pytestmark = pytest.mark.gpu

WRES = {1100: (64, 2), 1101: (128, 2), 1102: (32, 4)}      # id -> (TP, WGN): conv_wres.hip kWres
CAPS = (0, 3)                                              # yp_debug_max_workgroups: off, and few enough workgroups for several tiles each


def _lib():
    from yolo_puncture_amd.engine import load_library
    return load_library()


def _wres_paired(cout, tp, wgn):
    """conv_wres.hip's launcher, restated: channel blocks of at most 128 in whole fragments per channel wave; paired = an instantiation with
    at least 8 stores per wave and tile (wres_paired: <128,2> only), an even number of fragments per wave and whole 32-channel pairs"""
    nblk = (cout + 127) // 128
    q = 16 * wgn
    nb = ((cout + nblk - 1) // nblk + q - 1) // q * q
    stores = (tp // (16 * (8 // wgn))) * (8 // wgn)
    return stores >= 8 and (nb // q) % 2 == 0 and cout % 32 == 0


def _step(pair, shape, cfg, pick, cap):
    """Step (twice) every op of the plan under the forced id `cfg` that `pick` selects, in both engines -> {name: record}. Compared are the
    op's output tensor and, for a pwsp pair, the tensor of the pointwise result it stores beside it."""
    lib = _lib()
    wide, narrow, imc, outs = pair
    lib.yp_debug_force_conv_cfg(cfg)
    lib.yp_debug_max_workgroups(cap)
    try:
        ops = wide.plan(*shape)
        ops_n = narrow.plan(*shape)
        assert [(o["name"], o["kernel"], o["cfg"]) for o in ops] == [(o["name"], o["kernel"], o["cfg"]) for o in ops_n]   # no id, no symbol depends on the switch
        tinfo = {t["index"]: t for t in wide.tensors()}
        recs = {}
        for i, o in enumerate(ops):
            if o["kind"] == "head" or not pick(o):
                continue
            outs_t = [o["out"][0]] + ([ops[o["pre"]]["out"][0]] if o["pre"] >= 0 and o["pre_stored"] else [])
            got = []
            for rep in range(2):
                lib.yp_debug_last_store_form()         # (reading resets it: -1 below = the launch has one form only)
                wide.run_op(i, imc, outs[0])
                fw = lib.yp_debug_last_store_form()
                narrow.run_op(i, imc, outs[1])
                fn = lib.yp_debug_last_store_form()
                torch.cuda.synchronize()
                a = [wide.read_tensor(t) for t in outs_t]
                b = [narrow.read_tensor(t) for t in outs_t]
                print(f"  cfg {cfg} cap {cap} run {rep} {o['name']:30s} {o['kernel'][:40]:40s} out {o['out']} store form wide {fw} narrow {fn} "
                      f"differing elements {sum(int((x != y).sum()) for x, y in zip(a, b))}")
                assert fn <= 0, (o["name"], "the narrow engine launched the 16-byte form")
                for x, y in zip(a, b):
                    assert torch.equal(x, y), (cfg, cap, rep, o["name"], o["kernel"])
                got.append((fw, a))
            assert got[0][0] == got[1][0], o["name"]
            for x, y in zip(got[0][1], got[1][1]):
                assert torch.equal(x, y), (cfg, cap, o["name"], "two runs of one launch differ")
            recs[o["name"]] = {"form": got[0][0], "kernel": o["kernel"], "C": o["out"][2], "coff": o["out"][1], "f32": tinfo[o["out"][0]]["f32"],
                               "hw": tinfo[o["out"][0]]["shape"][:3]}
        return recs
    finally:
        lib.yp_debug_force_conv_cfg(-1)
        lib.yp_debug_max_workgroups(0)


# ---- conv_wres -------------------------------------------------------------------------------------------------------------------------------
_WRES_NAMES = {      # layers that must have run under the id (the plan decides; asserted, not assumed)
    1100: ("model.4.cv1", "model.4.cv2", "model.6.cv1", "model.7.cv1", "model.16.cv2", "model.10.attn.proj"),
    1101: ("model.4.cv1", "model.16.cv2"),           # (128-pixel tiles: only the 128-wide layers with short rows fit)
    1102: ("model.4.cv1", "model.4.cv2", "model.6.cv1", "model.7.cv1", "model.16.cv2", "model.10.attn.proj", "model.16.cv1", "model.13.cv2"),
}


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("cfg", sorted(WRES))
@pytest.mark.parametrize("shape", [(1, 256, 256), (2, 96, 160), (2, 256, 384)])
def test_conv_wres(shape, cfg, cap):
    """(1, 256, 256): 64 x 64 ... 8 x 8 maps, 256- and 512-wide layers = two and four channel blocks per tile, model.16.cv1's two row segments
    (folded upsample, id 1102), slices at channel offsets 256 (model.4.cv2) and 128 (model.13.cv2), the residual layer model.10.attn.proj.
    (2, 96, 160): M = 480 / 120 / 30 pixels: no multiple of the tile, TPe < TP. (2, 256, 384): 3072 pixels on P3, so that under the workgroup cap
    (8 tile lanes per channel block is the least the kernel's mapping admits) a lane walks 3 tiles of 128 pixels, 6 of 64, 12 of 32.
    model.23.proto.cv3 (32 channels = one fragment per wave) is the fallback."""
    tp, wgn = WRES[cfg]
    # (picked by the id the launch takes under the forced id: the plan of a shape that has run keeps the kernel NAME of its own pick)
    recs = _step(_pair("s", True, shape), shape, cfg, lambda o: o["cfg"] == cfg and o["kernel"] != "-", cap)
    assert set(_WRES_NAMES[cfg]) <= set(recs), (sorted(recs), "layers missing under the forced id")
    for n, r in recs.items():
        assert not r["f32"], n                           # (the family has no fp32 output)
        assert r["form"] == (1 if _wres_paired(r["C"], tp, wgn) else 0), (n, r)
    assert recs["model.4.cv1"]["form"] == recs["model.16.cv2"]["form"] == (1 if cfg == 1101 else 0)
    assert recs["model.23.proto.cv3"]["form"] == 0, "the odd-fragment fallback was not observed"
    if cfg != 1101:                                         # (the ids that keep the 8-byte form: residual layer and offset slice still agree)
        assert recs["model.10.attn.proj"]["form"] == 0 and recs["model.4.cv2"]["coff"] > 0
    if cap:
        b, h, w = recs["model.4.cv1"]["hw"]
        tiles = -(-(b * h * w) // tp)
        if shape == (2, 256, 384):
            assert tiles // 8 >= 3, tiles                  # every tile lane of model.4.cv1 walks at least 3 tiles


# ---- conv_dwpw_stream ------------------------------------------------------------------------------------------------------------------------
def _stream_case(shape, cap, want_form):
    recs = _step(_pair("s", True, shape), shape, -1, lambda o: o["kernel"] == "conv_dwpw_stream_kernel", cap)
    assert recs, "no op runs as conv_dwpw_stream_kernel"
    assert all(r["form"] == want_form for r in recs.values()), recs
    if cap:
        b, h, w = max((r["hw"] for r in recs.values()), key=lambda s: s[1] * s[2])
        assert b * -(-h // 8) * -(-w // 16) >= 2 * cap      # every workgroup runs at least 2 tiles (3 under cap 2)
    return recs


STREAM_CAPS = (0, 3, 2)      # (P3 is six tiles at both shapes: three workgroups walk two tiles each, two walk three)


@pytest.mark.parametrize("cap", STREAM_CAPS)
@pytest.mark.parametrize("shape", [(1, 160, 256), (1, 192, 256)])
def test_conv_dwpw_stream(shape, cap):
    """(1, 160, 256): P3 is 20 x 32 - partial tile rows, still within the two-thirds fill rule; (1, 192, 256): 24 x 32, exact tiles."""
    _stream_case(shape, cap, 1)


def test_conv_dwpw_stream_one_workgroup_per_cu_is_narrow():
    """YOLOP_DWPW_STREAM_ONE=1 (read once per process, hence the child): conv_dwpw_stream<8> has one fragment per wave = the 8-byte form."""
    env = dict(os.environ, YOLOP_DWPW_STREAM_ONE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "stream-one"], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "stream-one ok" in r.stdout


# ---- conv_halo_s2, c2f_fused -----------------------------------------------------------------------------------------------------------------
FRONT_SHAPES = [(2, 96, 160), (1, 64, 64)]      # model.1's output is 24 x 40 = 2.5 tiles across, 3 down (18 tiles); 16 x 16 = one tile across


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("shape", FRONT_SHAPES)
def test_c2f_fused(shape, cap):
    recs = _step(_pair("s", True, shape), shape, -1, lambda o: o["kernel"].startswith("c2f_fused_kernel"), cap)
    assert recs and all(r["form"] == 1 for r in recs.values()), recs


# ---- pwsp ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 96, 160), (1, 256, 256), (12, 64, 64)])
def test_pwsp(shape):
    """the plain form (id 1000), paired; the spatial forms (depthwise 3x3 / 7x7, SPPF pools), which keep the 8-byte form, agree as well. Not a
    persistent kernel: no workgroup cap. The first two shapes run 32-channel slices (one fragment pair per wave); at 12 frames the 512-wide
    layers give 96 workgroups of 64-channel slices (two pairs), which is what the bench shape runs."""
    pair = _pair("s", True, shape)
    recs = _step(pair, shape, -1, lambda o: o["kernel"].startswith("pwsp_kernel"), 0)
    sp = {r["kernel"] for r in recs.values()}
    assert any(k.endswith(",1>") for k in sp) and any(k.endswith(",2>") for k in sp) and any(k.endswith(",3>") for k in sp), sp
    assert all(r["form"] == -1 for r in recs.values()), recs      # (the spatial forms have the 8-byte form alone: nothing to report)
    assert any(k.startswith("pwsp_kernel<64,") for k in sp) == (shape[0] == 12), sp
    # the plain form: under the forced id 1000 every 1x1 that admits it launches as pwsp_kernel<NS,0> (the plan keeps the name of the op's own pick)
    plain = _step(pair, shape, 1000, lambda o: o["cfg"] == 1000 and o["kind"] == "conv" and o["kernel"] != "-", 0)
    assert plain and all(r["form"] == 1 for r in plain.values()), plain
    assert "model.10.attn.proj" in plain                    # (the residual layer: 16-byte residual reads)


# ---- fallback, chained -----------------------------------------------------------------------------------------------------------------------
def test_v10n_alignment_fallback_under_wres_ids():
    """v10-N, every op as its own kernel: its 80- / 48- / 16-channel layers miss the conditions of the paired form under the ids 1100+ and agree.
    Here id 1101 also takes the residual layer model.10.attn.proj and the folded-upsample layer model.16.cv1 (128 / 64 channels: paired)."""
    shape = (2, 96, 128)
    pair = _pair("n", True, shape, fuse=False)
    forms = []
    for cfg in sorted(WRES):
        recs = _step(pair, shape, cfg, lambda o: o["cfg"] == cfg and o["kernel"] != "-", 3 if cfg == 1101 else 0)
        forms += [(r["form"], r["C"] % 32 == 0) for r in recs.values()]
        if cfg == 1101:     # the paired instantiation with a residual (16-byte residual reads) and with two row segments (folded upsample)
            assert recs["model.10.attn.proj"]["form"] == 1 and recs["model.16.cv1"]["form"] == 1, recs
    print("v10-N (store form, 32-channel multiple) seen:", {f: forms.count(f) for f in set(forms)})
    assert any(f == 0 and not whole for f, whole in forms), "no narrow layer of v10-N took the 8-byte fallback under the conv_wres ids"
    assert all(f == 0 for f, whole in forms if not whole), forms
    assert any(f == 1 for f, _ in forms), "no launch of v10-N took the 16-byte form"


def test_chained_forward_equal():
    """the whole forward, also with few workgroups: det / idx of the two engines equal bit for bit"""
    shape = (2, 256, 384)
    wide, narrow, imc, _ = _pair("s", True, shape)
    lib = _lib()
    try:
        for cap in CAPS:
            lib.yp_debug_max_workgroups(cap)
            a, b = wide.forward(imc), narrow.forward(imc)
            torch.cuda.synchronize()
            for k in ("det", "idx"):
                assert torch.equal(a[k].cpu(), b[k].cpu()), (k, cap)
    finally:
        lib.yp_debug_max_workgroups(0)
        for e in _PAIRS.pop(("s", True, shape, True))[:2]:
            e.close()


if __name__ == "__main__" and sys.argv[1:] == ["stream-one"]:
    for cap_ in STREAM_CAPS:
        _stream_case((1, 160, 256), cap_, 0)
    print("stream-one ok")
