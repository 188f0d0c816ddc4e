"""The recurrent mLSTM step's checker (tests/mlstm_step_cases.py) on the host: an fp32 numpy
restatement of the recurrence passes it on every kernel case with 4x headroom, and each planted
defect fails it -- so a pass on the GPU means something."""
import numpy as np
import pytest
import torch

from tests import mlstm_step_cases as sc

RAGGED = [[1, 1, 1, 0, 0, 1, 1, 0, 1, 1, 1, 1], [1] * 12, [0] * 12]


def ragged_case(DQ, DV, carried=1):
    return sc.draw_case(3, 2, 12, DQ, DV, carried, seed=7 * DQ + carried, live=RAGGED)


@pytest.mark.parametrize("DQ,DV", sc.HEADS)
def test_fp32_restatement_passes_with_headroom(DQ, DV):
    cases = sc.case_set(DQ, DV) + [ragged_case(DQ, DV), ragged_case(DQ, DV, 0),
                                   sc.draw_case(2, 2, 200, DQ, DV, 1, seed=5)]
    worst = {}
    for c in cases:
        w = sc.check_step(c, *sc.numpy_step_fp32(c), what=str(c["key"][:7]))
        for k, x in w.items():
            worst[k] = max(worst.get(k, 0.0), x)
    print(f"head ({DQ}, {DV}): fp32 restatement, worst error / allowance {worst}")
    # h: c(t) >= DQ + t leaves a sound fp32 evaluation 4x headroom; the state's allowance
    # (4 + G_T) is only a few units at K = 1, where one 2-ulp exponential already takes a third
    assert worst["h"] <= 0.25 and max(worst.values()) <= 1.0, worst


def test_bf16_operands_are_rounded_on_both_sides():
    c = sc.draw_case(2, 2, 8, 32, 64, 1, seed=3, dtype=torch.bfloat16)
    h, C, n, m = sc.numpy_step_fp32(c)
    hb = torch.from_numpy(h).to(torch.bfloat16).float().numpy()   # a bf16 output
    sc.check_step(c, hb, C, n, m, out_unit=sc.U_BF16)
    with pytest.raises(AssertionError):
        sc.check_step(c, hb, C, n, m)   # an fp32 output is held to fp32


@pytest.mark.parametrize("defect", sc.DEFECTS)
@pytest.mark.parametrize("DQ,DV", sc.HEADS)
def test_planted_defect_fails(defect, DQ, DV):
    cases = sc.case_set(DQ, DV, Ks=(8, 64)) + [ragged_case(DQ, DV)]
    failed = 0
    for c in cases:
        try:
            sc.check_step(c, *sc.numpy_step_fp32(c, defect=defect))
        except AssertionError:
            failed += 1
    assert failed, f"defect {defect!r} passes the checker on every case"
    if defect != "mask_decay":   # (that one needs a held step: the ragged case)
        assert failed >= len(cases) // 2, (defect, failed, len(cases))


def test_held_rows_and_state():
    """A held step returns an exact zero row and leaves the state alone; the checker says so."""
    c = ragged_case(32, 64)
    h, C, n, m = sc.numpy_step_fp32(c)
    assert not h[2].any() and np.array_equal(C[2], c["c0"].numpy()[2])
    assert np.array_equal(m[2], c["m0"].numpy().reshape(3, 2)[2])
    h2 = h.copy()
    h2[0, :, 3] = 1e-3
    with pytest.raises(AssertionError):
        sc.check_step(c, h2, C, n, m)


@pytest.mark.parametrize("DQ,DV", sc.HEADS)
def test_case_set_reaches_both_branches(DQ, DV):
    """Both normaliser branches occur in every head size's set, in fp32 and bf16 operands."""
    for dt in (torch.float32, torch.bfloat16):
        hits = np.concatenate([sc.reference(x)["floor"].ravel() for x in sc.case_set(DQ, DV, dt)])
        share = np.nansum(hits) / hits.size
        assert 0.02 < share < 0.98, share
