"""The conv kernel forms stage by stage (csrc/conv.hip: conv_choice) as a table of cells, and the launchers' grid arithmetic in Python:
shared by tests/test_conv_forms_cpu.py (the table itself), tests/test_gpu_conv.py (one test id per cell) and
tests/test_conv_oracle_cpu.py (every problem the GPU tests use)."""
import contextlib
from collections import namedtuple

from conv_oracle import STAGES

# bbbp_conv_kernel_form (include/bbbp_hip.h)
F32, WINOGRAD, SPLIT, SPLIT_PIPE, C1_SPLIT, C1_SPLIT_PIPE, WGRAD_DENSE, WGRAD_SPARSE8, WGRAD_SPARSE4 = range(9)
FORM_NAMES = ["F32Direct", "Winograd", "SplitBf16", "SplitBf16Pipe", "Conv1SplitBf16", "Conv1SplitBf16Pipe", "WgradDense", "WgradSparse8",
              "WgradSparse4"]
FWD, DGRAD, WGRAD = 0, 1, 2
OP_NAMES = ["fwd", "dgrad", "wgrad"]

# pipe: bbbp_set_conv2_fwd_pipe(1); beside: bbbp_set_conv_wgrad_beside_encoder(1); big: the batch beside B = 1 (see big_batch below)
Cell = namedtuple("Cell", "op stage mask pipe beside form big")


def _cells():
    rows = [
        # forward.  big = the smallest B at which the launch has more work items than work-groups and the count is no multiple of the grid,
        # on 256 CUs (geometry() below restates each launcher; the test recomputes it for the device it runs on):
        #   f32 (launch_conv): items = B * hw / TH * ncb, TH = 256 / hw rows, ncb = cout / 64 (1 for cout = 32), grid = min(B * hw / TH, 512)
        #     S1 / W1: 64 B over 512 -> 9.  S2: 16 B over 512 -> 33.  W2: 32 B over min(16 B, 512) -> 33 (below, exactly 2 per group).
        #     W3: 16 B over min(4 B, 512): a multiple (4 per group) up to B = 128, ragged from 129 -- beyond the cap of 40: 40 it is.
        #   split-bf16 (launch_b3): items = B * hw / RL * nmb, RL = 256 / hw, nmb = cout / 32, grid 512 (pipelined: 256)
        #     S2: 32 B -> 17 (pipelined 9).  W2: 64 B -> 9 (pipelined 5).  W3: 32 B -> 17.
        #   Winograd (launch_wino): items = 16 B over 256 -> 17.  conv1 split-bf16 (bbbp_b3_conv1_fwd): 32 B over 512 -> 17.
        (FWD, "S1", 0, 0, 0, F32, 9), (FWD, "S1", 64, 0, 0, C1_SPLIT_PIPE, 17),
        (FWD, "S2", 0, 0, 0, F32, 33), (FWD, "S2", 1, 0, 0, WINOGRAD, 17), (FWD, "S2", 4, 0, 0, SPLIT, 17), (FWD, "S2", 5, 0, 0, SPLIT, 17),
        (FWD, "S2", 4, 1, 0, SPLIT_PIPE, 9),
        (FWD, "W1", 0, 0, 0, F32, 9), (FWD, "W1", 511, 0, 0, F32, 9),
        (FWD, "W2", 0, 0, 0, F32, 33), (FWD, "W2", 4, 0, 0, SPLIT, 9), (FWD, "W2", 4, 1, 0, SPLIT_PIPE, 5),
        (FWD, "W3", 0, 0, 0, F32, 40), (FWD, "W3", 4, 0, 0, SPLIT, 17), (FWD, "W3", 4, 1, 0, SPLIT, 17),     # no pipelined kernel for 32 x 32 maps
        # data gradient (same launchers, the channel roles swapped: ncb = cin / 64 or 1, nmb = cin / 32)
        #   f32: S2 16 B over 512 -> 33.  W2 16 B over 512 -> 33.  W3 8 B over min(4 B, 512): exactly 2 per group up to B = 128 -> the cap, 40.
        #   split-bf16: S2 16 B over 512 -> 33.  W2 32 B -> 17.  W3 16 B -> 33.  Winograd: 8 B over 256 -> 33.
        (DGRAD, "S2", 0, 0, 0, F32, 33), (DGRAD, "S2", 2, 0, 0, WINOGRAD, 33), (DGRAD, "S2", 8, 0, 0, SPLIT, 33),
        (DGRAD, "W2", 0, 0, 0, F32, 33), (DGRAD, "W2", 8, 0, 0, SPLIT, 17),
        (DGRAD, "W3", 0, 0, 0, F32, 40), (DGRAD, "W3", 8, 0, 0, SPLIT, 33),
        # weight gradient: strips of two rows, B * hw / 2, over the groups of one (input block, output block) pair -- big = strips no multiple
        # of the groups: S1 64 B over 512 -> 9.  S2 32 B over 256 -> 9 (288).  W1 64 B over 256 -> 5 (320).  W2 32 B over 64 -> 3 (96).
        # W3: 16 B over 16, never ragged -> 3.
        (WGRAD, "S1", 0, 0, 0, F32, 9), (WGRAD, "S1", 32, 0, 0, C1_SPLIT, 9),
        (WGRAD, "S2", 0, 0, 0, F32, 9), (WGRAD, "S2", 16, 0, 0, WGRAD_DENSE, 9), (WGRAD, "S2", 144, 0, 0, WGRAD_SPARSE8, 9),
        (WGRAD, "S2", 400, 0, 0, WGRAD_SPARSE4, 9), (WGRAD, "S2", 144, 0, 1, WGRAD_SPARSE4, 9),
        (WGRAD, "W1", 0, 0, 0, F32, 5), (WGRAD, "W1", 511, 0, 0, F32, 5),
        (WGRAD, "W2", 0, 0, 0, F32, 3), (WGRAD, "W2", 16, 0, 0, WGRAD_DENSE, 3), (WGRAD, "W2", 144, 0, 0, WGRAD_SPARSE8, 3),
        (WGRAD, "W2", 400, 0, 0, WGRAD_SPARSE4, 3),
        (WGRAD, "W3", 0, 0, 0, F32, 3), (WGRAD, "W3", 16, 0, 0, F32, 3), (WGRAD, "W3", 144, 0, 0, WGRAD_SPARSE8, 3),     # no dense form for 32 x 32 maps
        (WGRAD, "W3", 400, 0, 0, WGRAD_SPARSE4, 3),
    ]
    return [Cell(*r) for r in rows]


CELLS = _cells()
UNSUPPORTED = [(DGRAD, "S1"), (DGRAD, "W1")]        # bbbp_conv_kernel_form answers -1: no data gradient of a 3-channel stage
CAP = 40


def cell_id(c):
    return f"{c.stage}-{OP_NAMES[c.op]}-{FORM_NAMES[c.form]}-mask{c.mask}" + ("-pipe" if c.pipe else "") + ("-beside" if c.beside else "")


def cells(op=None):
    return [c for c in CELLS if op is None or c.op == op]


def _persistent_grid(want, nmb, nwork):            # csrc/common.h
    grid = want
    if grid >= 8 * nmb:
        grid -= grid % (8 * nmb)
    if grid > nwork:
        grid = nwork - nwork % nmb
    return max(grid, nmb)


def geometry(c, B, cus):
    """(work items, work-groups that share them) of the cell's launch at batch B on a device of ``cus`` compute units, under default knobs."""
    cin, cout, hw = STAGES[c.stage]
    if c.op == WGRAD:
        strips = B * hw // 2
        if cin == 3:
            groups = min(max(cus * 2 // (cout // 32), 1), strips)
        else:
            groups = min(max(cus // ((cin // 32) * (cout // 64)), 1), strips)
        return strips, groups
    mout = cout if c.op == FWD else cin                # channels the launch writes
    if c.form == F32:
        strips = B * hw // (256 // hw)
        return strips * max(mout // 64, 1), min(strips, 2 * cus)
    if c.form in (SPLIT, SPLIT_PIPE):
        nmb = mout // 32
        nwork = B * (hw // (256 // hw)) * nmb
        return nwork, _persistent_grid(cus * (1 if c.form == SPLIT_PIPE else 2), nmb, nwork)
    if c.form == WINOGRAD:
        ncb = mout // 32
        nwork = B * 8 * ncb
        return nwork, max(min(cus - cus % ncb, nwork), ncb)
    assert c.form == C1_SPLIT_PIPE, c
    return B * 32, _persistent_grid(cus * 2, 1, B * 32)


def ragged(c, B, cus):
    nwork, grid = geometry(c, B, cus)
    return nwork > grid and nwork % grid != 0


def big_batch(c, cus=256):
    """The smallest B <= CAP whose launch is ragged (weight gradient of W3: never; 3), else CAP."""
    return next((B for B in range(2, CAP + 1) if ragged(c, B, cus)), 3 if (c.op, c.stage) == (WGRAD, "W3") else CAP)


@contextlib.contextmanager
def selected(L, c):
    """Set the cell's mask and preferences, check that conv_choice answers the cell's form, restore both."""
    cin, cout, hw = STAGES[c.stage]
    old = L.bbbp_get_conv_winograd()
    assert L.bbbp_set_conv_winograd(c.mask) == 0
    old_pipe, old_beside = L.bbbp_set_conv2_fwd_pipe(c.pipe), L.bbbp_set_conv_wgrad_beside_encoder(c.beside)
    try:
        got = L.bbbp_conv_kernel_form(c.op, cin, cout, hw)
        assert got == c.form, f"{cell_id(c)}: conv_choice answers {FORM_NAMES[got] if got >= 0 else got}"
        yield
    finally:
        L.bbbp_set_conv2_fwd_pipe(old_pipe)
        L.bbbp_set_conv_wgrad_beside_encoder(old_beside)
        L.bbbp_set_conv_winograd(old)


def wants_wide(c):
    """The ``wide`` inputs go to every split-bf16, sparse and Winograd cell, and to the f32 cell under mask 0 of each stage and op."""
    return c.form != F32 or c.mask == 0


def problems():
    """Every (stage, B, kind) the GPU tests build an oracle for, each once."""
    out = []
    for c in CELLS:
        out += [(c.stage, 1, "plain"), (c.stage, c.big, "plain")]
        if wants_wide(c):
            out.append((c.stage, 2, "wide"))
        if c.op != FWD:
            out.append((c.stage, 2, "plain"))
        elif c.stage.startswith("W"):
            out.append((c.stage, 2, "flat"))
    return sorted(set(out))
