"""The masked-scan checker (tests/scan_mask_cases.py) judged on the CPU: its premise, its
definition, the mutants it must reject, and the argument validation of the masking options."""
import numpy as np
import pytest
import torch

from oracle import lucy_scan as oscan
from tests import scan_cases as sc
from tests import scan_mask_cases as mc

CASES = [(T, D, name) for T, D in mc.SHAPES for name in mc.MASKS]


def _case(T, D, name, dtype="f32"):
    case = mc.base_case(T, D, dtype)
    dh_last, masks = mc.draw_extras(T, D, dtype)
    return case, masks[name], dh_last


def test_premise_fp32_oracle_within_a_quarter_of_C():
    """The fp32 oracle against the fp64 oracle on every compacted row of every case stays within
    C / 4 (x 1.02): compaction moves no row out of the regime C was measured in.  Measured worst
    3.9e-7 (f32, T 65, D 72, all_live, row 1, s_last) against C / 4 = 5.1e-7."""
    worst = (0.0, None)
    for T, D, name in CASES:
        case, mask, dh_last = _case(T, D, name)
        for b in range(mc.B):
            rc = mc.row_case(case, mask, dh_last, b, name)
            if rc is None:
                continue
            m = sc.check(rc, sc.oracle_fp32(rc))
            for k, v in m.items():
                if k != "out" and v > worst[0]:
                    worst = (v, (T, D, name, b, k))
                assert v <= (1.0 if k == "out" else sc.C / 4 * 1.02), (T, D, name, b, k, v)
    print(f"fp32 oracle on compacted rows: worst {worst[0]:.2e} at {worst[1]} (C/4 = {sc.C / 4:.2e})")


@pytest.mark.parametrize("T,D,name", [c for c in CASES if c[0] in (5, 65, 130) and c[1] != 72 or c[:2] == (65, 72)])
def test_identity_steps_equal_the_compacted_oracle(T, D, name):
    """The definition: a step-by-step loop with identity steps at held frames equals the
    unmasked oracle on each row's live frames, scattered back (1e-12 of each tensor's scale)."""
    case, mask, dh_last = _case(T, D, name)
    loop = mc.identity_loop(case, mask, dh_last)
    ref = mc.compacted_reference(case, mask, dh_last, name)
    for k, v in ref.items():
        np.testing.assert_allclose(loop[k], v, rtol=0, atol=1e-12 * max(np.abs(v).max(), 1.0), err_msg=k)
    assert not mc.row_failures(mc.row_metrics(case, mask, dh_last, loop, name))


def _unmasked(case, dh_last):
    """The mutant that ignores the mask: the unmasked oracle on the full rows."""
    g = sc.oracle_gates(case)
    out, s = oscan.lucy_scan_fwd(g, case["h0"], case["s0"])
    d = case["dout"].astype(np.float64)
    d[:, -1] += dh_last
    dg, dh0, ds0 = oscan.lucy_scan_bwd(g, case["h0"], case["s0"], d, case["ds_last"])
    return {"out": out, "s_last": s, "h_last": out[:, -1], "dgates": dg, "dh0": dh0, "ds0": ds0,
            "dbias": dg.sum(1)}


def test_checker_rejects_the_mutants():
    T, D = 130, 64
    case, mask, dh_last = _case(T, D, "random")
    assert not mc.row_failures(mc.row_metrics(case, mask, dh_last, mc.identity_loop(case, mask, dh_last), "random"))
    # the mask ignored
    got = _unmasked(case, dh_last)
    ref = mc.compacted_reference(case, mask, dh_last, "random")
    live = mask.astype(bool)
    print(f"mask ignored: out off by {np.abs(got['out'] - ref['out'])[live].max():.2f}, "
          f"s_last by {np.abs(got['s_last'] - ref['s_last']).max():.1f}")
    bad = {k for _, k in mc.row_failures(mc.row_metrics(case, mask, dh_last, got, "random"))}
    assert {"out", "s_last", "h_last", "held_out", "held_dgates", "dh0", "ds0"} <= bad, bad
    assert any(k.startswith("dgates/") for k in bad)
    # a held frame's dout let into the Gh chain
    got = mc.identity_loop(case, mask, dh_last, held_dout=True)
    bad = {k for _, k in mc.row_failures(mc.row_metrics(case, mask, dh_last, got, "random"))}
    assert "dh0" in bad and any(k.startswith("dgates/") for k in bad), bad
    assert not {"out", "s_last", "h_last"} & bad
    # dh_last dropped (it has decayed away before it reaches dh0 of rows this long: the last
    # live steps' gate gradients show it)
    got = mc.identity_loop(case, mask, np.zeros_like(dh_last))
    bad = {k for _, k in mc.row_failures(mc.row_metrics(case, mask, dh_last, got, "random"))}
    assert {"dgates/" + n for n in sc.PLANES} <= bad and not {"out", "s_last", "h_last"} & bad, bad
    # dh_last added onto dout at T - 1, not at the last live frame: lost wherever T - 1 is held
    case, mask, dh_last = _case(T, D, "prefix")
    assert not mask[1, -1] and mask[1].any() and mask[0, -1]
    moved = dict(case, dout=case["dout"].astype(np.float64))
    moved["dout"][:, -1] += dh_last
    got = mc.identity_loop(moved, mask, np.zeros_like(dh_last))
    fails = mc.row_failures(mc.row_metrics(case, mask, dh_last, got, "prefix"))
    assert {(1, "dgates/" + n) for n in sc.PLANES} <= set(fails), fails
    assert not [k for k in fails if k[0] == 0], fails   # row 0 ends live: the same there


def test_zero_gradient_does_not_pass():
    """An all-zero dgates passes the rule on at most half of the elements of every plane of the
    compacted (130, 64) random rows (measured: at most 0.26), so 'zero gradient everywhere'
    cannot slip through as 'zero gradient at held frames'."""
    case, mask, dh_last = _case(130, 64, "random")
    worst = 0.0
    for b in range(mc.B):
        rc = mc.row_case(case, mask, dh_last, b, "random")
        for g in range(7):
            worst = max(worst, sc.zero_plane_share(rc, g))
    print(f"zero_plane_share on the compacted rows: at most {worst:.2f}")
    assert worst <= 0.5


def test_module_gradient_restatement_error():
    """The yardstick of test_gpu_masked_module.test_hold_parameter_gradients: torch_ref.lucyrnn64
    on each row's live frames, run in fp32 on the CPU, against the same in fp64, relative L2 per
    parameter.  The GPU test allows 4 x these figures (the factor of scan_cases.C: hardware rsq /
    rcp / exp2 and another order of composition), computed on the same inputs.  Measured here:
    from 8.1e-8 (output_proj.bias) to 1.0e-6 (tracks.0.0.linear.weight) on
    (40, 128, 5, 3, 32, 70) and from 7.7e-8 to 8.5e-7 (the same two) on (10, 48, 17, 2, 12, 23);
    the gate projections sit at 4e-7 .. 1e-6, the LayerNorms at 3e-7 .. 5e-7."""
    for cfg in mc.MODULE_CASES:
        Din, D, Bn, L, V, T = cfg
        p, x, masks, w = mc.module_inputs(*cfg)
        g64 = mc.ref_param_grads(p, x, masks, w, L, D, torch.float64)
        g32 = mc.ref_param_grads(p, x, masks, w, L, D, torch.float32)
        err = {k: mc.rel_l2(g32[k], g64[k]) for k in g64}
        print(f"{cfg}: fp32 restatement rel L2 " + ", ".join(f"{k} {v:.1e}" for k, v in err.items()))
        assert all(np.linalg.norm(v) > 0 for v in g64.values())
        assert 1e-8 < min(err.values()) and max(err.values()) < 1e-4, err


def test_mask_mode_and_masking_validation():
    import statecatcher_amd as sca
    from statecatcher_amd import _lib, model, ops, torch_library
    from tests.tframe_ref import model_from
    m = model_from(None, 2, 8, 64, 5)
    assert m.mask_mode == "ignore"
    cfg = sca.LucyRNNConfig(input_dim=8, hidden_dim=64, num_layers=1, vocab_size=5,
                            kernel_impl="triton", fused_ops=True, layer_norm=False)
    cfg.mask_mode = "hold"
    assert sca.LucyRNNtriton(cfg).mask_mode == "hold"
    cfg.mask_mode = "skip"
    with pytest.raises(ValueError, match="mask_mode"):
        sca.LucyRNNtriton(cfg)
    del cfg.mask_mode
    assert model.ASRModel(None, cfg, 5, 8, 0).masking == "zero"
    held = model.ASRModel(None, cfg, 5, 8, 0, masking="hold")
    assert held.masking == "hold" and held.encoder.mask_mode == "hold"
    with pytest.raises(ValueError, match="masking"):
        model.ASRModel(None, cfg, 5, 8, 0, masking="keep")
    with pytest.raises(NotImplementedError):
        model.ASRModel(None, model.build_rwkv_config(8, 5, 64, 1), 5, 8, 0, masking="hold")
    with pytest.raises(NotImplementedError):
        model.ASRModel(None, model.build_xlstm_config(8, 5), 5, 8, 0, masking="hold")
    # the mask argument of the ops: shape and device are checked before anything is launched
    with pytest.raises(ValueError, match=r"\[B,T\]"):
        ops.scan_mask(torch.ones(2, 5), 2, 6, torch.device("cpu"))
    with pytest.raises(ValueError, match=r"\[B,T\]"):
        ops.scan_mask(torch.ones(2, 6, 1), 2, 6, torch.device("cpu"))
    with pytest.raises(ValueError, match="is on"):
        ops.scan_mask(torch.ones(2, 6), 2, 6, torch.device("meta"))
    for mk in (torch.ones(2, 6, dtype=torch.bool), torch.full((2, 6), 3), torch.full((2, 6), 0.5)):
        u8 = ops.scan_mask(mk, 2, 6, torch.device("cpu"))
        assert u8.dtype == torch.uint8 and u8.is_contiguous() and bool((u8 == 1).all())
    # the new symbols in the binding derived from the header, and in the dispatcher's op list
    assert {"sc_lucy_scan_fwd_masked", "sc_lucy_scan_bwd_masked"} <= set(_lib.EXPORTED)
    assert len(_lib._SIGS["sc_lucy_scan_fwd_masked"][1]) == len(_lib._SIGS["sc_lucy_scan_fwd"][1]) + 3
    assert len(_lib._SIGS["sc_lucy_scan_bwd_masked"][1]) == len(_lib._SIGS["sc_lucy_scan_bwd"][1]) + 2
    assert _lib.ABI_VERSION == 14
    assert {"lucy_scan_masked_fwd", "lucy_scan_masked_bwd"} <= set(torch_library.OPS)


def test_null_mask_is_einval():
    """A NULL mask is refused before anything is launched (callers without a mask use the old
    entry points)."""
    from statecatcher_amd import _lib
    lib = _lib.load()
    n = None
    assert lib.sc_lucy_scan_fwd_masked(n, 0, n, n, n, n, n, n, n, n, n, 1, 1, 1, 1, 1, 1, 64, 1, 1,
                                       n, n) == _lib.SC_EINVAL
    assert b"null mask" in lib.sc_last_error()
    assert lib.sc_lucy_scan_bwd_masked(n, 0, n, n, n, n, n, n, n, n, n, n, 1, 1, 1,
                                       1, 1, 1, 64, 1, 1, 1, 1, 1, 64, n) == _lib.SC_EINVAL
    assert b"null mask" in lib.sc_last_error()
