"""The RNN-T parity checker (tests/rnnt_cases.py) judged on the CPU: the fp32 restatement of the
kernels' algorithm measures C and C_sm, the fp64 oracle passes against itself, and every seeded
fault of the fp64 gradient is rejected on a case the GPU tests run."""
import numpy as np
import pytest

from tests import rnnt_cases as rc


def _case_id(case):
    return "-".join(str(k) for k in case["key"])


CPU_CASES = list(rc.cpu_cases())


def _oracle_result(case, **kw):
    ref = rc.reference(case)
    return {"nll": ref["nll"].copy(),
            "grad": rc.assemble(case, kw.get("gb", ref["gb"]), kw.get("gy", ref["gy"]),
                                kw.get("sm", ref.get("sm")), kw.get("lab"))}


def _rejected(case, got):
    return rc.failures(rc.check(case, got))


def test_launch_rules_cover_every_instantiation():
    """The case list reaches K = 16, 8, 4, 2, 1, one to 16 waves, the one-to-two-wave step, every
    nvec of both element sizes and the scalar loop (rules restated from csrc/rnnt.hip)."""
    ks = {rc.ab_halo_k(u) for u in rc.HALO_UMAX}
    assert ks == {16, 8, 4, 2, 1} and rc.ab_halo_k(1008) == 0
    assert [rc.ab_halo_k(u) for u in (767, 768, 895, 896, 959, 960, 991, 992, 1007)] == \
        [16, 8, 8, 4, 4, 2, 2, 1, 1]
    assert (rc.ab_waves(47), rc.ab_waves(48), rc.ab_waves(95), rc.ab_waves(96)) == (1, 2, 2, 3)
    assert {rc.ab_waves(u) for u in rc.HALO_UMAX} >= {1, 2, 3, 14, 15, 16}
    assert [rc.row_nvec(v, "f32") for v in rc.ROW_V["f32"]] == [1, 2, 3, 4, 0, 0, 0]
    assert [rc.row_nvec(v, "bf16") for v in rc.ROW_V["bf16"]] == [1, 3, 4, 0]
    assert rc.row_nvec(256, "f32", aligned=False) == 0


def test_fp32_restatement_measures_C():
    """The measurements behind C and C_sm, asserted: each is 4 x the worst value of the fp32
    restatement over the case list (C: the whole restatement with no row term granted; C_sm: the
    row stage alone on the fp64 occupancies)."""
    worst = {"unit_c": (0.0, None), "unit_sm": (0.0, None)}
    for case in CPU_CASES:
        got = rc.restate_fp32(case)
        m = rc.check(case, got)
        assert m["nll"] <= 1.0 and m["nonzero"] == 0, (case["key"], m)
        c = rc.measure(case, got)["unit_c"]
        if c > worst["unit_c"][0]:
            worst["unit_c"] = (c, case["key"])
        if case["logits"]:
            s = rc.measure(case, rc.restate_fp32(case, exact_arcs=True))["unit_sm"]
            if s > worst["unit_sm"][0]:
                worst["unit_sm"] = (s, case["key"])
    print(f"fp32 restatement: worst {worst}; C = {rc.C:g}, C_sm = {rc.C_SM:g}")
    for name, const in (("unit_c", rc.C), ("unit_sm", rc.C_SM)):
        assert worst[name][0] <= const / 4 * 1.02, (name, worst[name])
        assert worst[name][0] >= const / 8, f"{name}: the constant is over 8x the measurement"


@pytest.mark.parametrize("case", CPU_CASES, ids=_case_id)
def test_oracle_passes_against_itself(case):
    m = rc.check(case, _oracle_result(case))
    assert m == {"nll": 0.0, "nonzero": 0, "grad": 0.0}, m


def test_blocked_sequences_are_infinite_with_zero_rows():
    """What the reference says of a sequence with every path blocked: nll = +inf, no gradient;
    the neighbours keep theirs.  A huge finite nll or an occupancy of order 1 is rejected."""
    for kind in ("final_blank", "label_column"):
        for logits in (False, True):
            case = rc.masked_case(kind, logits)
            ref = rc.reference(case)
            assert np.isposinf(ref["nll"][1]) and np.isfinite(ref["nll"][[0, 2]]).all()
            assert not ref["gb"][1].any() and not ref["gy"][1].any()
            assert ref["gb"][0].any() and ref["gb"][2].any()
            got = _oracle_result(case)
            got["nll"][1] = 6.9e29
            assert "nll" in _rejected(case, got)
            gb = ref["gb"].copy()
            gb[1, :33, :10] = -0.3
            assert "nonzero" in _rejected(case, _oracle_result(case, gb=gb))


FAULT_CASES = [rc.halo_case(95), rc.halo_case(96), rc.halo_case(768), rc.diag_case(33),
               rc.diag_case(64), rc.mid_case()]


@pytest.mark.parametrize("case", FAULT_CASES, ids=_case_id)
@pytest.mark.parametrize("m", [1, -3, 40])
def test_rejects_one_diagonal_scaled(case, m):
    """A wrong offset index at a re-centring boundary: one diagonal's occupancies x 2^m."""
    ref = rc.reference(case)
    per = 2 * rc.ab_halo_k(case["x"].shape[2] - 1)
    t, u = np.meshgrid(np.arange(case["x"].shape[1]), np.arange(case["x"].shape[2]), indexing="ij")
    for n in (per - 1, per):
        on = (t + u == n)[None]
        gb, gy = (np.where(on, g * 2.0 ** m, g) for g in (ref["gb"], ref["gy"]))
        assert "grad" in _rejected(case, _oracle_result(case, gb=gb, gy=gy)), n


@pytest.mark.parametrize("case", [rc.halo_case(48), rc.halo_case(95), rc.halo_case(96)],
                         ids=_case_id)
def test_rejects_a_stale_wave_seam(case):
    """The value at the wave seam u = 48 taken from the previous diagonal (a halo lane that missed
    its exchange)."""
    ref = rc.reference(case)
    for name in ("gb", "gy"):
        g = ref[name].copy()
        g[:, 1:, 48] = ref[name][:, :-1, 48]
        if np.array_equal(g, ref[name]):       # Umax = 48 has no label arc at u = 48
            assert name == "gy" and case["x"].shape[2] == 49
            continue
        assert "grad" in _rejected(case, _oracle_result(case, **{name: g})), name


@pytest.mark.parametrize("case", [rc.diag_case(16), rc.diag_case(17),
                                  rc.row_case("f32", 512, 77, True),
                                  rc.row_case("bf16", 512, 511, False)], ids=_case_id)
def test_rejects_the_next_label(case):
    """The label column gathered at y[u+1]."""
    lab = rc.label_index(case)
    nxt = lab.copy()
    for b in range(lab.shape[0]):
        Ub = int(case["ll"][b])
        nxt[b, :max(Ub - 1, 0)] = case["labels"][b, 1:Ub]
    assert (nxt != lab).any()
    assert _rejected(case, _oracle_result(case, lab=nxt))


@pytest.mark.parametrize("case", [rc.row_case("f32", 256, 0, True), rc.row_case("f32", 1024, 77, True),
                                  rc.row_case("bf16", 512, 0, True),
                                  rc.row_case("f16", 2048, 77, True)], ids=_case_id)
def test_rejects_a_dropped_vector(case):
    """The log-sum-exp taken over V - 4 columns (the row's last fp32 vector dropped)."""
    x = case["x"].astype(np.float64)
    lse = np.log(np.exp(x[..., :-4]).sum(-1, keepdims=True))
    assert "grad" in _rejected(case, _oracle_result(case, sm=np.exp(x - lse)))


@pytest.mark.parametrize("case", [rc.halo_case(48), rc.diag_case(15), rc.u0_case(17),
                                  rc.row_case("f32", 512, 77, True, compact=False)], ids=_case_id)
def test_rejects_a_nonzero_padding_row(case):
    got = _oracle_result(case)
    Tb = int(case["fl"][1])
    assert Tb < case["x"].shape[1]
    got["grad"][1, Tb:, 0, 1] = 1e-30
    assert _rejected(case, got) == {"nonzero": case["x"].shape[1] - Tb}
    got = _oracle_result(case)
    got["grad"][1, 0, 0, :] += 1e-30          # a valid row, a column no arc uses
    if not case["logits"]:
        assert "nonzero" in _rejected(case, got)


def test_tiny_arcs_are_a_floor_not_a_skip():
    """Arcs below 2^-100 may come back as 0 or anything up to 2^-99 |s|, nothing larger."""
    case = rc.sharp_case(100, 130, 70)
    ref = rc.reference(case)
    tiny = (np.abs(ref["gb"]) < rc.TINY) & (ref["gb"] != 0)
    assert tiny.any() and not tiny.all()
    assert not _rejected(case, _oracle_result(case, gb=np.where(tiny, 0.0, ref["gb"])))
    assert "grad" in _rejected(case, _oracle_result(case, gb=np.where(tiny, -2.0 ** -97, ref["gb"])))
