"""CPU: the host-side plans of the GEMM and conv entry points answer exactly what they answered before they were gathered into one plan
function each (csrc/gemm.hip: gemm_plan, csrc/conv.hip: conv_choice).

tests/plan_tables.json holds, for every case listed below, the values of bbbp_gemm_workspace_bytes, bbbp_gemm_folds_asum and
bbbp_conv3x3_workspace_bytes.  It was recorded with tools/record_plan_tables.py from a build of the commit BEFORE that refactor
(`BBBP_LIB=<that build's libbbbp_hip.so> python tools/record_plan_tables.py`), never from the code under test; the same command against that
build reproduces the file byte for byte.  Without a device the library plans for 256 CUs, the count of an MI355X, so the table is the same
on a CPU-only machine and on the GPU machine (default knobs: no BBBP_* variable set)."""
import ctypes
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "plan_tables.json")

FC, IMG_FLAT, COMB, FUS_HID, DFF = 128, 65536, 256, 128, 2048


def engine_gemm_cases():
    """Every product the engine issues for bench configurations 2-5: F in {167, 2048} (one head of 167, 256 heads of 8), B in
    {32, 256, 512, 4096}; each Linear as forward (B, N, K), input gradient (B, K, N) and weight gradient (N, K, B), the attention
    products per head, the folded projections, and the image-FC products."""
    out = []
    for F, NH in ((167, 1), (2048, 256)):
        D = F // NH
        linears = [(3 * F, F), (2 * F, F), (F, F), (DFF, F), (F, DFF), (FC, F), (FC, IMG_FLAT), (FUS_HID, COMB), (COMB, FUS_HID),
                   (256, COMB), (128, 256), (64, 128), (1, 64)]
        for B in (32, 256, 512, 4096):
            for N, K in linears:
                out += [(B, N, K, 1), (B, K, N, 1), (N, K, B, 1)]
            out += [(B, B, D, NH), (B, D, B, NH)]                   # S = Q K^T | dP = dO V^T;  O = P V | dQ = dS K | dV = P^T dO | dK = dS^T Q
    return out


def boundary_gemm_cases():
    out = []
    # the 1.2 GFLOP limit of the small-product path: 2 * 1000 * 600 * K
    out += [(1000, 600, K, 1) for K in (999, 1000, 1001)] + [(500, 600, K, 2) for K in (999, 1000, 1001)]
    # K rules: split-K from 256, the 64 x 64 split-bf16 tile and the deep-K 128 tile from 512, the small-product path up to 8192
    for K in (31, 32, 255, 256, 511, 512, 1023, 1024, 8191, 8192, 8193):
        for M, N in ((16, 16), (64, 64), (128, 128), (128, 512), (256, 256), (512, 128), (1024, 167), (4096, 167), (1024, 1024),
                     (2048, 2048), (2176, 2048), (2432, 2048)):
            out += [(M, N, K, 1), (M, N, K, 8)]
    # 128 x 128 tile counts around 3/4 of the CUs (192) and around the CU count (256), 64 x 64 counts around the split-bf16 window (640)
    for t in (191, 192, 193, 255, 256, 257):
        out += [(128 * t, 128, K, 1) for K in (64, 256, 512)] + [(128, 128, K, t) for K in (64, 256, 512)]
    for t in (319, 320, 321, 509, 510, 511, 512):
        out += [(64 * t, 128, K, 1) for K in (511, 512, 2048)]
    # small-product path: wave-tile and wave counts (4096 tiles, 16384 waves), tiny head dimensions, grid limits
    out += [(1024, 1024, 16, 1), (1024, 1040, 16, 1), (2048, 2048, 16, 1), (2048, 2064, 16, 1), (4096, 4096, 16, 1), (64, 64, 8, 64),
            (64, 8, 64, 8), (64, 8, 64, 7), (16, 16, 16, 65535), (16, 16, 16, 65536), (16, 16, 16, 70000), (0, 16, 16, 1), (16, 0, 16, 1),
            (16, 16, 0, 1), (16, 16, 16, 0)]
    return out


def gemm_cases():
    seen, out = set(), []
    for c in engine_gemm_cases() + boundary_gemm_cases():
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def conv_cases():
    """(B, cin, cout, H, W): the five supported stage shapes and one unsupported shape."""
    shapes = [(3, 32, 128), (32, 64, 64), (3, 64, 128), (64, 128, 64), (128, 256, 32), (16, 16, 32)]
    return [(B, cin, cout, hw, hw) for cin, cout, hw in shapes for B in (1, 32, 512, 4096)]


def load_library(path):
    L = ctypes.CDLL(path)
    L.bbbp_gemm_workspace_bytes.restype = ctypes.c_size_t
    L.bbbp_gemm_workspace_bytes.argtypes = [ctypes.c_int] * 4
    L.bbbp_gemm_folds_asum.restype = ctypes.c_int
    L.bbbp_gemm_folds_asum.argtypes = [ctypes.c_int] * 4
    L.bbbp_conv3x3_workspace_bytes.restype = ctypes.c_size_t
    L.bbbp_conv3x3_workspace_bytes.argtypes = [ctypes.c_int] * 5
    return L


def compute_tables(L):
    """The table's content from a loaded library: rows of [M, N, K, batch, workspace bytes, folds asum] and [B, cin, cout, H, W, bytes]."""
    return {"gemm": [[*c, L.bbbp_gemm_workspace_bytes(*c), L.bbbp_gemm_folds_asum(*c)] for c in gemm_cases()],
            "conv": [[*c, L.bbbp_conv3x3_workspace_bytes(*c)] for c in conv_cases()]}


def _recorded():
    with open(TABLE) as f:
        return json.load(f)


def test_table_covers_the_listed_cases():
    rec = _recorded()
    assert [tuple(r[:4]) for r in rec["gemm"]] == gemm_cases()
    assert [tuple(r[:5]) for r in rec["conv"]] == conv_cases()
    # the table exercises every answer, not one side of each rule
    assert {r[5] for r in rec["gemm"]} == {0, 1}
    assert any(r[4] > 0 for r in rec["gemm"]) and any(r[4] == 0 and r[5] == 0 and min(r[:4]) > 0 for r in rec["gemm"])
    assert (512, 128, 65536, 1) in gemm_cases() and (128, 65536, 512, 1) in gemm_cases() and (512, 65536, 128, 1) in gemm_cases()


def test_gemm_plans_match_the_recorded_table():
    from bbbp_amd import _lib
    L = _lib.lib()
    for M, N, K, batch, ws, folds in _recorded()["gemm"]:
        assert L.bbbp_gemm_workspace_bytes(M, N, K, batch) == ws, (M, N, K, batch)
        assert L.bbbp_gemm_folds_asum(M, N, K, batch) == folds, (M, N, K, batch)


def test_conv_workspace_matches_the_recorded_table():
    from bbbp_amd import _lib
    L = _lib.lib()
    for B, cin, cout, H, W, ws in _recorded()["conv"]:
        assert L.bbbp_conv3x3_workspace_bytes(B, cin, cout, H, W) == ws, (B, cin, cout, H, W)
