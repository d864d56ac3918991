"""The fixtures and references of tests/vecchia_edge_ref.py without a GPU: on every rung and case the conditions under which the
GPU comparison leaves no datum out and no bound is vacuous (cap gaps above 1e-9, every local system positive definite, cond(A) of
the trend's normal matrix below 1e3), the reference's own floor in the length-scale class of the information, the sampled
reference of the tall case against vecchia_reference on a problem small enough for both, and the helpers of the sum identities."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import dense_chains as dc   # noqa: E402
from tests import test_gpu_vecchia_trend as tgt   # noqa: E402
from tests import vecchia_edge_ref as ve   # noqa: E402
from tests import vecchia_grad_ref as vgr   # noqa: E402
from tests import vecchia_ref as vr   # noqa: E402
from tests import vecchia_trend_ref as vtr   # noqa: E402

COND_MAX = 1e3


# ---------------------------------------------------------------------------------------------------------------------
# 1. the ladder
# ---------------------------------------------------------------------------------------------------------------------
def test_the_ladder_has_the_sizes_it_is_for():
    run, strip, tree = 8, 64, 256
    two = [s for s in map(ve.sizes_of, ve.LADDER) if len(s) == 2]
    n0s = {s[0] for s in two}
    assert {1, 7, 8, 9} <= n0s and {1, 8, 9} <= {s[1] for s in two}             # below, on and past a run; one-site processes
    assert any(n0 % strip == 0 for n0 in n0s) and any(n0 % strip == 1 for n0 in n0s) and any(n0 % strip == strip - 1 for n0 in n0s)
    assert any(n0 % run != 0 and n0 > run for n0 in n0s)                        # row0 = ceil(n0 / 8) differs from n0 / 8
    totals = {sum(s) for s in map(ve.sizes_of, ve.LADDER)}
    assert {tree, tree + 1, 2 * tree, 2 * tree + 1} <= totals and min(totals) == 1
    tall, info_tall = sum(ve.TALL_SIZES), ve.INFO_TALL_SIZES
    assert -(-tall // tree) > tree                                              # a second trip of every k_*_sum loop
    assert sum(-(-n // run) for n in info_tall) > tree                          # and of k_vecchia_info_part's rows


@pytest.mark.parametrize("label", ve.LADDER)
def test_rung_conditions(label):
    pb, ref = ve.rung(label), ve.value_reference(label)
    tr = ve.trend_reference(label)
    cond = np.linalg.cond(tr["A"])
    print(f"{label}: smallest gap {ref['gap'].min():.2e}, smallest variance {ref['var'].min():.3e}, k_max {ref['k_max']}, "
          f"n_capped {ref['n_capped']}, n_empty {ref['n_empty']}, trend {ve.trend_kinds(ve.sizes_of(label))} cond(A) {cond:.1f}")
    assert ref["gap"].min() > 1e-9                      # numpy and the device agree on every set: no datum left out
    assert ref["info"] == 0 and np.all(ref["var"] > 0)
    assert cond < COND_MAX
    assert tr["p"] == sum(3 if n >= 8 else 1 for n in ve.sizes_of(label))
    assert np.array_equal(tr["count"], ref["count"]) and ref["k_max"] <= 8
    assert len(pb["ranks"]) == sum(ve.sizes_of(label))
    if sum(ve.sizes_of(label)) >= 64:
        assert ref["n_capped"] > 0                      # the cap binds: the select pass runs


def test_a_process_of_one_site_takes_no_linear_design():
    pb = ve.rung("1+1")
    with pytest.raises(ValueError, match="process 0 has 1 data sites for 3 regressors"):
        ve.trend_design(pb, ("linear", "constant"))
    assert ve.trend_kinds((1, 1)) == ("constant", "constant") and ve.trend_kinds((7, 9)) == ("constant", "linear")
    assert ve.trend_kinds((8, 8)) == ("linear", "linear")


def test_a_rung_takes_its_rows_of_the_shared_derivative_matrices():
    for label in ("7+9", "uni9"):
        pb = ve.rung(label)
        own = vgr.derivative_matrices(pb["params"], pb["coords"], pb["metric"])
        for a, b in zip(ve.ladder_dS(label), own):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("label", ve.LADDER + [ve.INFO_TALL])
def test_reference_floor(label):
    """the procedure of tests/test_vecchia_info_host.py: test_reference_floor -- what halving the step changes"""
    if label == ve.INFO_TALL:
        sets, ref, half, npar = ve.info_tall_sets(), ve.info_tall_reference(), ve.info_tall_reference(0.5), 11
        assert sets["gap"].min() > 1e-9 and sets["info"] == 0 and sets["n_capped"] > 0
        print(f"{label}: smallest gap {sets['gap'].min():.2e}, k_max {sets['k_max']}")
    else:
        ref, half, npar = ve.info_reference(label), ve.info_reference(label, 0.5), ve.npar_of(ve.rung(label))
    e = dc.class_errors(dc.normalised(half, ref), npar)
    print(f"{label}: floor of the reference exact {e['exact']:.2e} length scale {e['len']:.3e} nu {e['nu']:.2e}, live slots "
          f"{ve.info_live(ref).tolist()}")
    tol = ve.info_tol(label)
    assert e["exact"] == 0.0                            # the exact block expressions do not see the step
    assert 10.0 * e["len"] <= tol["len"]                # the bound of the GPU module is at least ten floors
    assert e["nu"] < tol["nu"] / 10
    live = ve.info_live(ref)
    assert set(live.tolist()) <= set(range(npar)) and np.array_equal(live, ve.info_live(half))
    # every slot has information, but: a process of one site has none on its own nu and length scale, and two co-located sites
    # alone none on the cross pair's either
    sizes = ve.INFO_TALL_SIZES if label == ve.INFO_TALL else ve.sizes_of(label)
    dead = {1: {1, 2}}.get(sizes[0], set()) if npar == 4 else (({2, 5} if sizes[0] == 1 else set()) | ({4, 7} if sizes[1] == 1 else set())
                                                               | ({3, 6} if sizes == (1, 1) else set()))
    assert live.tolist() == [s for s in range(npar) if s not in dead]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the helpers of the sum identities
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_sum_and_gram_helpers():
    s, b = ve.exact_sum([1e16, 1.0, -1e16, 1.0])
    assert s == 2.0 and b == ve.SUM_FACTOR * ve.U * (2e16 + 2.0)
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((300, 5))
    G, B = ve.gram_of_rows(rows)
    assert np.array_equal(G, G.T) and np.all(B > 0) and np.all(np.abs(G - rows.T @ rows) <= B)
    dropped = rows[:-1]                                 # one row less: far outside the bound
    assert ve.gram_excess(dropped.T @ dropped, G, B) > 1e6
    assert ve.gram_excess(rows.T @ rows, G, B) <= 1.0


@pytest.mark.parametrize("label", ve.LADDER)
def test_the_gram_matrix_is_recovered_from_the_outputs(label):
    """G -> (yy, beta, Cov(beta)) -> G within GRAM_RECOVERY |G_ab|: what the inversion in the GPU test's identity costs"""
    tr = ve.trend_reference(label)
    G = ve.recovered_gram(tr["out5"], tr["beta"], tr["cov"])
    rel = np.max(np.abs(G - tr["G"]) / np.abs(tr["G"]))
    print(f"{label}: recovery of G, max relative {rel:.2e}")
    assert rel <= ve.GRAM_RECOVERY
    rows = ve.trend_rows(tr["z"], tr["X"], tr["prior"] + tr["own"], tr["mean"], tr["prior"] - tr["var"], tr["g"])
    Gr, B = ve.gram_of_rows(rows)
    assert ve.gram_excess(tr["G"], Gr, B) <= 1.0        # the reference's own G against its own rows


# ---------------------------------------------------------------------------------------------------------------------
# 3a. the sampled reference
# ---------------------------------------------------------------------------------------------------------------------
def test_sampled_reference_is_the_full_reference_on_300_sites():
    pb = ve.problem((150, 150), n_sites=150)
    X, _ = ve.constant_design(pb)
    full = vtr.vecchia_trend_reference(pb["params"], pb["coords"], pb["values"], X, pb["metric"], pb["ranks"], pb["max_dist"],
                                       pb["caps"])
    want = vgr.vecchia_grad_reference(pb["params"], pb["coords"], pb["values"], pb["metric"], full)
    got = ve.sampled_reference(pb, np.arange(300), X=X)
    assert np.array_equal(got["count"], full["count"]) and full["n_capped"] > 100 and full["n_empty"] > 0
    assert np.array_equal(got["capped"], vr.conditioning_sets(*vr.stacked_distances(pb["coords"], pb["metric"]), pb["ranks"],
                                                              pb["max_dist"], pb["caps"])[2])
    assert np.array_equal(got["gap"], full["gap"])
    for key in ("mean", "var", "g"):
        d = np.max(np.abs(got[key] - full[key]))
        print(f"sampled against full, {key}: {d:.2e}")
        assert d <= 1e-13
    d = np.max(np.abs(got["score"][:, :11] - want["score"][:, :11]) / np.maximum(np.abs(want["score"][:, :11]), 1.0))
    print(f"sampled against full, scores: {d:.2e}")
    assert d <= 1e-13


def test_tall_sample_and_its_reference():
    N = sum(ve.TALL_SIZES)
    s = ve.tall_sample()
    assert len(s) == ve.TALL_SAMPLE and np.array_equal(s, np.unique(s)) and s[-1] == N - 1
    assert {0, ve.TALL_SIZES[0] - 1, ve.TALL_SIZES[0], N - 1, 255, 256, 65535, 65536} <= set(s.tolist())
    assert np.array_equal(s, ve.tall_sample())                       # fixed
    ref = ve.tall_reference()
    close = int(np.count_nonzero(ref["gap"] < 1e-9))
    ktot = ref["count"].sum(axis=1)
    print(f"tall sample: {close} data with a cap gap below 1e-9, smallest gap {ref['gap'].min():.2e}, capped "
          f"{np.count_nonzero(ref['capped'])}, empty {np.count_nonzero(ktot == 0)}, k_max {ktot.max()}, smallest variance "
          f"{ref['var'].min():.3e}")
    assert close <= 2
    assert np.all(ref["var"] > 0) and np.all(np.isfinite(ref["score"]))
    assert np.count_nonzero(ref["capped"]) > 64 and ktot.max() == 6 and np.all(ref["count"] <= 3)   # the caps bind and hold
    small = ve.tall_sample((9, 8), 12)                               # the rule on a size without the four fixed indices
    assert len(small) == 12 and {0, 8, 9, 16} <= set(small.tolist())


# ---------------------------------------------------------------------------------------------------------------------
# 4. trend width
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,caps", ve.WIDE_CASES)
def test_wide_designs_are_well_conditioned(ps, caps):
    pb = tgt.problem()
    ref = tgt.reference(pb, ve.wide_trend(*ps), 0.5, caps)
    cond = np.linalg.cond(ref["A"])
    print(f"p = {ps} caps {caps}: cond(A) {cond:.1f}, k_max {ref['k_max']}, smallest gap {ref['gap'].min():.2e}")
    assert ref["p"] == sum(ps) and [f.shape[1] for f in ref["F"]] == list(ps)
    assert cond < COND_MAX and ref["gap"].min() > 1e-9 and ref["info"] == 0
    assert ref["k_max"] == 2 * caps[0]


def test_wide_design_under_full_conditioning_is_well_conditioned():
    from sif_xco2_cokriging_amd import vecchia
    pb = tgt.small_problem()
    for ordering in ("random", "hilbert"):
        ranks = vecchia.ordering_ranks(pb["coords"], ordering, 1)
        ref = tgt.reference(pb, ve.wide_trend(8, 8), 2.0, (0, 0), ranks=ranks, key=ordering)
        cond = np.linalg.cond(ref["A"])
        print(f"p = (8, 8) on 40 + 25, {ordering}: cond(A) {cond:.1f}")
        assert cond < COND_MAX and ref["k_max"] == 64 and ref["p"] == 16
