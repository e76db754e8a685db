"""The paired channel order of the 16-byte conv stores (csrc/kernel_util.h: paired_channel, acc_channel), restated in Python. No GPU.

A lane of a 16x16 MFMA accumulator holds A-rows fc*4 .. fc*4+3 of its pixel (fc = lane >> 4). Row i of fragment a of the fragment pair
(2j, 2j+1) is filled with the weights of output channel j*32 + (i >> 2)*8 + (a & 1)*4 + (i & 3), so lane group fc holds channels
j*32 + fc*8 + 0..3 in fragment 2j and + 4..7 in fragment 2j+1: eight consecutive channels at a multiple of 8 = one 16-byte store."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parents[1] / "yolo-puncture_amd" / "csrc"


def paired_channel_issue(a, i):
    """the issue's statement of the map: A-row i of fragment a -> channel (fragments (2j, 2j+1) form pair j)"""
    return (a >> 1) * 32 + (i >> 2) * 8 + (a & 1) * 4 + (i & 3)


def paired_channel(row):
    """kernel_util.h's form, on the row of a weight image whose 32-row blocks are fragment pairs"""
    return (row & ~31) | ((row & 12) << 1) | ((row & 16) >> 2) | (row & 3)


def acc_channel(a, fc, wide):
    return (a >> 1) * 32 + fc * 8 + (a & 1) * 4 if wide else a * 16 + fc * 4


def test_header_states_the_same_map():
    text = " ".join((CSRC / "kernel_util.h").read_text().split())
    assert "paired_channel(int row) { return (row & ~31) | ((row & 12) << 1) | ((row & 16) >> 2) | (row & 3); }" in text
    assert re.search(r"acc_channel\(int a, int fc, bool wide\) \{ return wide \? \(a >> 1\) \* 32 \+ fc \* 8 \+ \(a & 1\) \* 4 : a \* 16 \+ fc \* 4; \}", text)


def test_row_form_equals_fragment_form():
    for a in range(16):
        for i in range(16):
            assert paired_channel(a * 16 + i) == paired_channel_issue(a, i)


def test_bijection_on_every_32_channel_block():
    for j in range(8):
        rows = range(j * 32, j * 32 + 32)
        assert sorted(paired_channel(r) for r in rows) == list(rows)


def test_lane_group_holds_eight_consecutive_channels():
    for j in range(8):
        for fc in range(4):
            held = []
            for a in (2 * j, 2 * j + 1):                   # the lane's four accumulator values of fragment a are A-rows fc*4 + 0..3
                held += [paired_channel_issue(a, fc * 4 + r) for r in range(4)]
            first = held[0]
            assert first % 8 == 0 and first == j * 32 + fc * 8
            assert held == list(range(first, first + 8))   # in register order: fragment 2j's four, then fragment 2j+1's
            assert acc_channel(2 * j, fc, True) == first and acc_channel(2 * j + 1, fc, True) == first + 4


def test_narrow_form_is_the_natural_order():
    for a in range(8):
        for fc in range(4):
            assert acc_channel(a, fc, False) == a * 16 + fc * 4
