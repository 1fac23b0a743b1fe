"""CPU: the C-ABI library loads, exports every symbol include/bbbp_hip.h declares, and the product path refuses to
run without a GPU instead of falling back to anything."""
import ctypes

import pytest
import torch

import bbbp_amd
from bbbp_amd import _lib, ops


def test_library_exports_every_declared_symbol():
    declared = _lib.declared_symbols()
    assert len(declared) >= 25
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} is declared in include/bbbp_hip.h but not exported by libbbbp_hip.so"
    # every declared symbol has a ctypes signature and vice versa
    assert sorted(_lib._SIGNATURES) == declared
    assert _lib.lib().bbbp_abi_version() == 1


def test_descriptor_and_plan_functions_without_gpu():
    L = _lib.lib()
    d = _lib.MixedDesc(batch=512, fingerprint_size=167, nhead=1, num_layers=6, dim_feedforward=2048, training=1,
                       dropout_p=0.1, seed=1, need_input_grad=0)
    assert L.bbbp_mixed_num_params(ctypes.byref(d)) == 106 == len(list(bbbp_amd.MixedInputModel(167, 128).parameters()))
    ws = L.bbbp_mixed_workspace_bytes(ctypes.byref(d))
    assert 0.9e9 < ws < 4e9                 # ~1.0 GB of saved activations + scratch at B = 512
    bad = _lib.MixedDesc(batch=4, fingerprint_size=167, nhead=8, num_layers=6, dim_feedforward=2048)
    assert L.bbbp_mixed_workspace_bytes(ctypes.byref(bad)) == 0
    assert b"divisible" in L.bbbp_last_error()
    assert L.bbbp_gemm_workspace_bytes(512, 128, 65536, 1) > 0          # split-K slabs for the image FC


def test_no_cpu_fallback():
    m = bbbp_amd.MixedInputModel(64, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 64), torch.zeros(2, 49152))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gemm(torch.zeros(2, 2), torch.zeros(2, 2))
    with pytest.raises(ValueError):
        bbbp_amd.MixedInputModel(64, 64)        # the reference's forward hard-codes 3x128x128


def test_module_surface_matches_reference_contract():
    m = bbbp_amd.MixedInputModel(167, 128)
    keys = list(m.state_dict().keys())
    assert keys[0] == "fingerprint_transformer.layers.0.self_attn.in_proj_weight"
    assert "image_cnn.7.weight" in keys and "attention_fusion.attention_heads.3.2.bias" in keys
    assert "fc.2.running_mean" in keys and "fc.2.num_batches_tracked" in keys and "fc.7.bias" in keys
    assert sum(p.numel() for p in m.parameters()) == 13_464_087
    assert m.nhead == 1 and bbbp_amd.MixedInputModel(64, 128).nhead == 8
    # parameters live in one flat buffer, in named_parameters order, and stay so after dtype/device moves
    from bbbp_amd.models import flat_view_of
    assert flat_view_of(list(m.parameters())) is not None
    m.float()
    assert flat_view_of(list(m.parameters())) is not None
    ds = bbbp_amd.MixedDataset([[1.0, 2.0]], [[3.0]], [0.5])
    fp, img, y = ds[0]
    assert len(ds) == 1 and fp.dtype == img.dtype == y.dtype == torch.float32 and y.dim() == 0


def test_overlapped_reducer_schedule_tiles_the_flat_gradient_buffer():
    """distributed.OverlappedGradAllReduce fixes its collective schedule at construction from the parameter layout alone (host
    side, no GPU): image-FC weight, encoder layers from the last to the first, the two remaining slices, the conv tensors --
    together exactly the flat buffer, once."""
    import bbbp_amd
    from bbbp_amd import distributed as D
    for cls, F, layers in ((bbbp_amd.MixedInputModel, 64, 6), (bbbp_amd.ConcatMixedInputModel, 167, 6), (bbbp_amd.TwoBranchConcatModel, 167, 0)):
        m = cls(F, 128)
        r = D.OverlappedGradAllReduce(m)
        sched = r.schedule()
        assert [b for _, b, _, _ in sched if b is not None and b != 1] == [0] + list(range(1 + layers, 1, -1))
        spans = sorted((lo, hi) for _, _, lo, hi in sched if hi > lo)
        total = sum(p.numel() for p in m.parameters())
        assert spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        w = m.image_cnn[7].weight
        assert (sched[0][3] - sched[0][2]) == w.numel() == 128 * 65536
        if layers:
            per_layer = sum(p.numel() for p in m.fingerprint_transformer.layers[0].parameters())
            assert all(hi - lo == per_layer for _, b, lo, hi in sched if b is not None and b >= 2)


def test_graph_replay_stays_off_while_any_reducer_is_alive():
    """closing one reducer must not switch HIP-graph replay back on under another live reducer -- the first reducer
    remembers the process's mode, the LAST one to close restores it (host side only: bbbp_set_graphs is a flag)."""
    import bbbp_amd
    from bbbp_amd import _lib, distributed as D
    L = _lib.lib()
    before = L.bbbp_set_graphs(1)                     # pretend the process runs with replay on
    try:
        m = bbbp_amd.TwoBranchConcatModel(167, 128)
        a, b = D.OverlappedGradAllReduce(m), D.OverlappedGradAllReduce(m)
        assert L.bbbp_set_graphs(0) == 0              # off while both live (the query sets 0, which is what it already is)
        a.close()
        assert L.bbbp_set_graphs(0) == 0              # still off: b is alive
        b.close()
        assert L.bbbp_set_graphs(1) == 1              # restored by the last close
        a.close(); b.close()                          # idempotent
        assert D._LIVE["count"] == 0
    finally:
        L.bbbp_set_graphs(before)


def test_round4_entry_points_validate_their_arguments_before_touching_the_gpu():
    """Argument errors are reported as BBBP_ERR_ARG with a message, before any HIP call (so: testable without a GPU)."""
    import ctypes
    from bbbp_amd import _lib
    L = _lib.lib()
    ERR_ARG = 1
    fake = ctypes.c_void_p(4096)                         # never dereferenced: validation comes first
    # multi-tensor AdamW: tensor count, null pointers, alignment of the flat buffers, 1-based step
    assert L.bbbp_adamw_step_multi(None, fake, fake, fake, 16, fake, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None) == ERR_ARG
    assert b"n_tensors" in L.bbbp_last_error()
    assert L.bbbp_adamw_step_multi(None, fake, fake, fake, 16, None, 2, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None) == ERR_ARG
    assert L.bbbp_adamw_step_multi(None, ctypes.c_void_p(4100), fake, fake, 16, fake, 2, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None) == ERR_ARG
    assert b"aligned" in L.bbbp_last_error()
    assert L.bbbp_adamw_step_multi(None, fake, fake, fake, 16, fake, 2, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, None) == ERR_ARG
    assert L.bbbp_adamw_step_multi(None, fake, fake, fake, 0, None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None) == 0          # empty: nothing to do
    assert L.bbbp_adamw_hyper_store(None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0) == ERR_ARG
    assert L.bbbp_adamw_step(None, fake, fake, fake, fake, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0) == ERR_ARG
    assert L.bbbp_adamw_step_deferred(None, fake, fake, fake, fake, 16, 8, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0) == ERR_ARG   # lo > hi
    # per-thread setters are plain flags
    assert L.bbbp_set_seed_base(None) == 0
    prev = L.bbbp_set_conv_wgrad_beside_encoder(1)
    assert L.bbbp_set_conv_wgrad_beside_encoder(prev) == 1
    # MLP profile: group count bound
    buf = (ctypes.c_ulonglong * 3)()
    assert L.bbbp_mlp_profile_groups(ctypes.cast(buf, ctypes.c_void_p), 5000) == ERR_ARG
    assert L.bbbp_mlp_profile_groups(None, 1) == ERR_ARG


def test_encoder_row_fold_and_ln_grad_entry_points_validate_their_arguments_before_touching_the_gpu():
    """bbbp_outproj_fold_fwd / _bwd, bbbp_ln_param_grad, bbbp_encoder_rows_fwd / _bwd: a null required pointer, an empty extent, an
    unsupported width and a malformed next projection are BBBP_ERR_ARG with a message before any HIP call; the optional arguments (bo, the
    next projection, stage 0 of the backward) are the only ones that may be NULL."""
    L = _lib.lib()
    ERR_ARG, FAKE = 1, 4096                              # never dereferenced: validation comes first

    def refused(rc, *words):
        msg = L.bbbp_last_error()
        return rc == ERR_ARG and all(w in msg for w in words)

    # ---- the predicates ----
    assert [L.bbbp_outproj_fold_supported(F, 1, 1) for F in (0, 1, 255, 256)] == [0, 1, 1, 0]
    assert [L.bbbp_outproj_fold_supported(167, 1, n) for n in (0, 1, 32, 33)] == [0, 1, 1, 0] and L.bbbp_outproj_fold_supported(64, 8, 6) == 0
    assert [L.bbbp_encoder_rows_supported(F, 1, 16) for F in (3, 4, 192, 193)] == [0, 1, 1, 0]
    assert [L.bbbp_encoder_rows_supported(167, 1, d) for d in (15, 16, 18, 2048)] == [0, 1, 1, 1] and L.bbbp_encoder_rows_supported(64, 0, 64) == 0

    # ---- fold forward: host lists of device pointers ----
    one, none = _lib.ptr_array([FAKE]), _lib.ptr_array([None])
    lists = [one] * 3 + [None] + [one] * 3                # win, bin, wo, bo (optional), wf, bf, wvt
    for F, layers in ((0, 1), (256, 1), (167, 0), (167, 33)):
        assert refused(L.bbbp_outproj_fold_fwd(None, layers, F, *lists), b"not supported"), (F, layers)
    for i in (0, 1, 2, 4, 5, 6):
        assert refused(L.bbbp_outproj_fold_fwd(None, 1, 167, *[None if j == i else a for j, a in enumerate(lists)]), b"null"), i
        assert refused(L.bbbp_outproj_fold_fwd(None, 1, 167, *[none if j == i else a for j, a in enumerate(lists)]), b"null"), i
    # ---- fold backward ----
    ptrs = [FAKE] * 5, [FAKE] * 4                         # tdw, tdb, wo, wvt, dz | g_outw, g_outb, g_inw_v, g_inb_v
    for F, B, lddz, word in ((0, 4, 8, b"not supported"), (256, 4, 256, b"not supported"), (167, 0, 167, b"B 0"), (167, 4, 166, b"lddz 166")):
        assert refused(L.bbbp_outproj_fold_bwd(None, F, B, *ptrs[0], lddz, *ptrs[1]), word), (F, B, lddz)
    for i in range(9):
        a = [None if j == i else FAKE for j in range(9)]
        assert refused(L.bbbp_outproj_fold_bwd(None, 167, 4, *a[:5], 167, *a[5:]), b"null"), i
    # ---- LayerNorm parameter gradients ----
    two = _lib.ptr_array([FAKE, FAKE])
    for n, rows, cols in ((0, 4, 4), (-1, 4, 4), (2, 0, 4), (2, 4, 0)):
        assert refused(L.bbbp_ln_param_grad(None, n, *[two] * 6, rows, cols), b"n %d, rows %d, cols %d" % (n, rows, cols))
    for i in range(6):
        assert refused(L.bbbp_ln_param_grad(None, 2, *[None if j == i else two for j in range(6)], 4, 4), b"null"), i
        assert refused(L.bbbp_ln_param_grad(None, 2, *[_lib.ptr_array([FAKE, None]) if j == i else two for j in range(6)], 4, 4), b"norm 1"), i

    # ---- row forward ----
    def fwd(**kw):
        d = _lib.EncoderRowsFwdDesc(B=37, F=167, DFF=2048, dropout_p=0.1, seed1=1, seed2=2, seed3=3)
        for name in _lib.ENCODER_ROWS_FWD_INPUTS + _lib.ENCODER_ROWS_FWD_OUTPUTS:
            setattr(d, name, FAKE)
        for k, v in kw.items():
            setattr(d, k, v)
        return L.bbbp_encoder_rows_fwd(None, ctypes.byref(d))

    assert refused(L.bbbp_encoder_rows_fwd(None, None), b"null descriptor")
    for name in _lib.ENCODER_ROWS_FWD_INPUTS + _lib.ENCODER_ROWS_FWD_OUTPUTS:
        assert refused(fwd(**{name: None}), b"null pointer"), name
    for B in (0, -3):
        assert refused(fwd(B=B), b"B %d" % B)
    for kw in (dict(F=3), dict(F=193), dict(DFF=15), dict(DFF=0)):
        assert refused(fwd(**kw), b"not supported"), kw
    for p in (-0.1, 1.0):
        assert refused(fwd(dropout_p=p), b"dropout_p"), p
    nxt = dict(wn=FAKE, bn=FAKE, outn=FAKE, nn=128, ldn=256, actn=1)
    for bad in (dict(nn=0), dict(nn=-1), dict(ldn=127), dict(bn=None), dict(outn=None)):
        assert refused(fwd(**{**nxt, **bad}), b"next projection"), bad

    # ---- row backward ----
    def bwd(**kw):
        d = _lib.EncoderRowsBwdDesc(B=37, F=167, DFF=2048, dropout_p=0.1, seed1=1, seed3=3, dyout=FAKE)
        for name in _lib.ENCODER_ROWS_BWD_INPUTS + _lib.ENCODER_ROWS_BWD_OUTPUTS:
            setattr(d, name, FAKE)
        for k, v in kw.items():
            setattr(d, k, v)
        return L.bbbp_encoder_rows_bwd(None, ctypes.byref(d))

    assert refused(L.bbbp_encoder_rows_bwd(None, None), b"null descriptor")
    for name in ("dyout",) + _lib.ENCODER_ROWS_BWD_INPUTS + _lib.ENCODER_ROWS_BWD_OUTPUTS:
        assert refused(bwd(**{name: None}), b"null pointer"), name
    assert refused(bwd(B=0), b"B 0")
    for kw in (dict(F=3), dict(F=193), dict(DFF=15)):
        assert refused(bwd(**kw), b"not supported"), kw
    assert refused(bwd(dropout_p=1.0), b"dropout_p")
    stage0 = ("dqkv_up", "win_up", "dz1_up")
    for given in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
        assert refused(bwd(**{stage0[i]: FAKE for i in given}), b"stage 0"), given
