"""CPU: which kernel form conv_choice (csrc/conv.hip) picks for every stage, op and mask of the table in tests/conv_cells.py, asked through
bbbp_conv_kernel_form -- host code only, the library loads without a device.  Default knobs: the BBBP_C* variables are read once per process,
so a run with one of them set is skipped, not judged."""
import os

import pytest

from bbbp_amd import _lib
from conv_oracle import STAGES
import conv_cells as cc

KNOBS = ["BBBP_C2_PIPE", "BBBP_C2_DGRAD_PIPE", "BBBP_B3_PROBE", "BBBP_C2_WGRAD_SPARSE_WAVES", "BBBP_C1_PIPE"]


@pytest.fixture(autouse=True)
def default_knobs():
    if any(k in os.environ for k in KNOBS):
        pytest.skip("a BBBP_C* form knob is set in the environment: the table holds for the defaults")


@pytest.mark.parametrize("cell", cc.CELLS, ids=cc.cell_id)
def test_form_of_cell(cell):
    L = _lib.lib()
    before = L.bbbp_get_conv_winograd()
    with cc.selected(L, cell):                         # asserts the form
        assert L.bbbp_get_conv_winograd() == cell.mask
    assert L.bbbp_get_conv_winograd() == before
    # both preferences are back at their defaults: setting 0 returns the previous value
    assert L.bbbp_set_conv2_fwd_pipe(0) == 0 and L.bbbp_set_conv_wgrad_beside_encoder(0) == 0


def test_table_covers_every_stage_op_and_form():
    assert {(c.op, c.stage) for c in cc.CELLS} | set(cc.UNSUPPORTED) == {(op, s) for op in (cc.FWD, cc.DGRAD, cc.WGRAD) for s in STAGES}
    assert {c.form for c in cc.CELLS} == set(range(9))
    assert len({cc.cell_id(c) for c in cc.CELLS}) == len(cc.CELLS)


def test_unsupported_answers_minus_one():
    L = _lib.lib()
    for op, stage in cc.UNSUPPORTED:
        assert L.bbbp_conv_kernel_form(op, *STAGES[stage]) == -1
    for mask in (0, 511):
        old = L.bbbp_get_conv_winograd()
        try:
            L.bbbp_set_conv_winograd(mask)
            assert L.bbbp_conv_kernel_form(cc.FWD, 16, 16, 32) == -1
            assert L.bbbp_conv_kernel_form(cc.FWD, 32, 64, 32) == -1           # a supported channel pair on another map size
            assert L.bbbp_conv_kernel_form(3, 32, 64, 64) == -1 and L.bbbp_conv_kernel_form(-1, 32, 64, 64) == -1
        finally:
            L.bbbp_set_conv_winograd(old)


def test_mask_round_trip_and_rejection():
    L = _lib.lib()
    old = L.bbbp_get_conv_winograd()
    try:
        for mask in (0, 1, 252, 511):
            assert L.bbbp_set_conv_winograd(mask) == 0 and L.bbbp_get_conv_winograd() == mask
        assert L.bbbp_set_conv_winograd(512) != 0 and L.bbbp_get_conv_winograd() == 511       # rejected: the mask stays
        assert L.bbbp_set_conv_winograd(-1) != 0 and b"mask" in L.bbbp_last_error()
    finally:
        L.bbbp_set_conv_winograd(old)
    assert L.bbbp_get_conv_winograd() == old


def test_default_mask_forms():
    """Under the default mask (252) the flagship's stages run what the engine's plans were measured with."""
    L = _lib.lib()
    if "BBBP_CONV_WINOGRAD" in os.environ or L.bbbp_get_conv_winograd() != 252:
        pytest.skip("the mask is not at its default")
    want = {(cc.FWD, "S1"): cc.C1_SPLIT_PIPE, (cc.WGRAD, "S1"): cc.C1_SPLIT, (cc.FWD, "S2"): cc.SPLIT, (cc.DGRAD, "S2"): cc.SPLIT,
            (cc.WGRAD, "S2"): cc.WGRAD_SPARSE8, (cc.WGRAD, "W3"): cc.WGRAD_SPARSE8, (cc.FWD, "W1"): cc.F32}
    for (op, stage), form in want.items():
        assert L.bbbp_conv_kernel_form(op, *STAGES[stage]) == form, (op, stage)


def test_big_batches_follow_the_launch_arithmetic():
    """The table's second batch per cell is what geometry() gives for 256 compute units; B = 1 never has more work than groups."""
    for c in cc.CELLS:
        assert c.big == cc.big_batch(c, 256), (cc.cell_id(c), cc.big_batch(c, 256))
        if c.big < cc.CAP and (c.op, c.stage) != (cc.WGRAD, "W3"):
            assert cc.ragged(c, c.big, 256) and not cc.ragged(c, 1, 256)
