"""Host side of the register-weights instances of the stride-2 halo conv (conv_halo_s2.hip): which instance a launch of id 500 / 501 takes,
its LDS need and the validity predicate, through the host-only mode of yp_debug_conv_s2; the family's id range, the plan's kernel names and
the library's symbols. No GPU needed."""
import pytest

from yolo_puncture_amd.engine import Engine, conv_families, conv_s2_admits, load_library

RING4 = 3 * 19 * 1024 + 1024        # three halo slots of a 4-row tile (9 x 33 pixel rows -> 19 KiB) + the 1-KiB landing zone
RING8 = 3 * 36 * 1024 + 1024        # 8-row tile: 17 x 33 pixel rows -> 36 KiB per slot
SLAB = 9 * 64 * 64                  # a 32-channel chunk of the 3x3 weights of a 64-channel block
K = "conv_halo_s2_kernel<"


def test_family_keeps_its_five_ids():
    """the register-weights instances are launch forms of ids 500 / 501, no ids of their own"""
    assert (500, 5) in conv_families()
    assert conv_s2_admits(505, 1, 64, 64, 64, 128) == (False, 0, "") and conv_s2_admits(499, 1, 64, 64, 64, 128) == (False, 0, "")


@pytest.mark.parametrize("cin", [32, 64])
def test_instance_and_lds_of_ids_500_501(cin):
    """Cin = 32 / 64 (at most 144 weight registers): the launch holds the halo ring alone - or one chunk of a 128-channel block, which is
    staged whole and is more than the 4-row ring; with weights in LDS the ring and Cin / 32 chunks"""
    nch = cin // 32
    for cout, tile, lds in ((64, "1,2,4,2,3", RING4), (96, "1,2,4,2,3", RING4), (100, "2,2,2,4,3", 2 * SLAB), (128, "2,2,2,4,3", 2 * SLAB),
                            (256, "2,2,2,4,3", 2 * SLAB)):
        assert conv_s2_admits(501, 2, 80, 80, cin, cout) == (True, lds, f"{K}{tile},false,false,false,{nch}>"), (cin, cout)
        assert conv_s2_admits(501, 2, 80, 80, cin, cout, lds_weights=True) == (True, RING4 + nch * SLAB, f"{K}1,2,4,2,3,false,false,false>")
    assert 2 * SLAB > RING4
    assert conv_s2_admits(500, 2, 80, 80, cin, 128) == (True, RING8, f"{K}2,2,4,2,3,false,false,false,{nch}>")
    # residual and fp32-output variants exist for every instance; both at once for none (as before)
    assert conv_s2_admits(501, 2, 80, 80, cin, 128, res=True)[2] == f"{K}2,2,2,4,3,true,false,false,{nch}>"
    assert conv_s2_admits(501, 2, 80, 80, cin, 64, out_f32=True)[2] == f"{K}1,2,4,2,3,false,true,false,{nch}>"
    assert conv_s2_admits(500, 2, 80, 80, cin, 64, res=True)[2] == f"{K}2,2,4,2,3,true,false,false,{nch}>"
    assert not conv_s2_admits(501, 2, 80, 80, cin, 128, True, True)[0]


def test_register_bound():
    """9 taps x (Cin / 32) chunks x 2 fragments x 4 VGPRs <= 144: Cin = 96 (216) and 128 (288) keep their weights in LDS, with the LDS
    bound that goes with it; ids 502 - 504 have no register instance"""
    assert conv_s2_admits(501, 2, 80, 80, 96, 128) == (False, RING4 + 3 * SLAB, "") and RING4 + 3 * SLAB > 160 * 1024      # (166 KB: as before)
    ok, lds, name = conv_s2_admits(501, 2, 80, 80, 128, 128)
    assert (ok, lds, name) == (False, RING4 + 4 * SLAB, "") and lds > 160 * 1024
    assert not conv_s2_admits(500, 2, 80, 80, 96, 128)[0]
    for cfg, tile in ((502, "2,2,4,1,3"), (503, "1,2,4,1,3")):
        for cin in (32, 64):
            ok, lds, name = conv_s2_admits(cfg, 2, 80, 80, cin, 128)
            assert ok and name == f"{K}{tile},false,false,false>" and lds == (RING8 if cfg == 502 else RING4) + (cin // 32) * SLAB // 2
    assert not conv_s2_admits(504, 2, 80, 80, 32, 128)[0] and not conv_s2_admits(504, 2, 80, 80, 64, 256)[0]      # (181 KB and more, as before)


def test_eight_row_tile_fits_for_cin_64():
    """model.3 of v10-S at the bench shape: the 8-row tile with LDS weights needs 182 KB and is refused, with register weights it fits"""
    shape = (32, 160, 160, 64, 128)
    ok_l, lds_l, _ = conv_s2_admits(500, *shape, lds_weights=True)
    ok_r, lds_r, _ = conv_s2_admits(500, *shape)
    assert not ok_l and lds_l == RING8 + 2 * SLAB and lds_l > 160 * 1024
    assert ok_r and lds_r == RING8 and lds_r <= 160 * 1024
    assert conv_s2_admits(501, *shape)[0] and conv_s2_admits(501, *shape, lds_weights=True)[0]


def test_other_conditions_are_unchanged():
    """odd maps, channel counts that are no multiple of 32 / 4, a 64-channel block on a 32-channel layer, tiles that cover more than
    1.5 x the map: refused whichever instance would launch"""
    for cfg in (500, 501):
        for lds_weights in (False, True):
            assert not conv_s2_admits(cfg, 1, 63, 64, 32, 128, lds_weights=lds_weights)[0]
            assert not conv_s2_admits(cfg, 1, 64, 64, 48, 128, lds_weights=lds_weights)[0]
            assert not conv_s2_admits(cfg, 1, 64, 64, 32, 126, lds_weights=lds_weights)[0]
            assert not conv_s2_admits(cfg, 1, 64, 64, 32, 32, lds_weights=lds_weights)[0]
            assert not conv_s2_admits(cfg, 1, 4, 8, 32, 128, lds_weights=lds_weights)[0]      # 2 x 4 output pixels under a 4 x 16 / 8 x 16 tile
            assert conv_s2_admits(cfg, 1, 16, 32, 32, 128, lds_weights=lds_weights)[0]


@pytest.mark.parametrize("cfg", [500, 501])
def test_plan_names_real_symbols(cfg):
    """v10-S at (1, 256, 256) under the forced id: model.3 (64 -> 128) launches the register-weights instance - the 128-channel block under
    501 - and model.17 (128 -> 128, four chunks) does not; every kernel the plan names is a symbol of the library, and the LDS-weights
    symbols are as they were"""
    from test_kernel_symbols import CXXFILT, NM, _kernel_symbols
    lib = load_library()
    e = Engine("s", 80, False, "bf16", 0)
    try:
        lib.yp_debug_force_conv_cfg(cfg)
        e.plan(1, 32, 32)
        ops = {o["name"]: o for o in e.plan(1, 256, 256)}
    finally:
        lib.yp_debug_force_conv_cfg(-1)
        e.close()
    tile = "2,2,4,2,3" if cfg == 500 else "2,2,2,4,3"
    assert ops["model.3"]["cfg"] == cfg and ops["model.3"]["kernel"] == f"{K}{tile},false,false,false,2>", ops["model.3"]
    assert ops["model.17"]["cfg"] != cfg, ops["model.17"]
    took = [o for o in ops.values() if o["cfg"] == cfg and o["kernel"] != "-"]
    if NM and CXXFILT:
        syms = _kernel_symbols(lib._name)
        for o in took:
            assert o["kernel"] in syms, o
        for t in ("1,2,4,2,3", "2,2,4,2,3", "2,2,2,4,3"):
            for tail in ("false,false,false", "true,false,false", "false,true,false"):        # plain, residual, fp32 output x one / two chunks
                for nch in (1, 2):
                    assert f"{K}{t},{tail},{nch}>" in syms
                assert (f"{K}{t},{tail}>" in syms) == (t != "2,2,2,4,3")
