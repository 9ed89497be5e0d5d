"""tests/field_contract.py without a GPU: the checks that hold gsr_field.hip to its fp32 contract pass on the numpy restatements
(field_values_host, level_surface_host) at every case the GPU file runs, with no hit skipped, and fail on restatements that are wrong
in the ways a kernel goes wrong: an expf off by more than its allowance, another summation order, a contracted product, a dropped slot,
a reordered interpolation."""
import numpy as np
import pytest
import torch

import field_cases as FC
import field_contract as CT
import levelset_cases as LC
from autovfx_amd import field, levelset
from test_field import random_case
from test_levelset import LEVELS, SHAPES, shape_case

F = np.float32
TINY = np.finfo(F).tiny


# ---- the cases (tests/test_field_contract_gpu.py runs the kernels on the same ones) ----
def far_case():
    """Samples spread by 3 sigma of the cloud: many e in the denormal range, many exactly 0."""
    c = random_case(1000, 16, 40, seed=3)
    c["x"] = (c["x"] + np.random.default_rng(0).normal(0, 3 * np.abs(c["x"]).std(), c["x"].shape)).astype(F)
    return c


def edge_case():
    """test_field_gpu.py's far sample (q > 1e8), sample at the centre (q == 0) and scale at get_covariance's clamp (entries of 1e8)."""
    c = random_case(65, 3, 4, seed=12, bad_slots=False)
    c["M"][3] = (c["M"][3].astype(np.float64) / np.linalg.norm(c["M"][3].astype(np.float64), axis=0) * np.array([5.0, 5.0, 1e8])).astype(F)
    c["idx"][:] = np.array([0, 1, 2])
    c["idx"][0], c["idx"][1], c["idx"][2], c["idx"][3] = 0, 1, 3, 3
    c["x"][0] = c["centers"][0] + F(3000.0)
    c["x"][1] = c["centers"][1]
    c["x"][2] = c["centers"][3] + F(0.01)
    c["x"][3] = c["centers"][3]
    return c


def nonfinite_field_case():
    c = random_case(257, 17, 40, seed=21)
    c["x"][3, 0] = np.nan
    c["x"][4, 1] = np.inf
    c["centers"][5] = np.nan
    c["M"][6, 0, 0] = np.inf
    c["M"][7, 1, 2] = np.nan
    c["min_scaling"][8] = np.nan
    return c


def fixture_field_case(name):
    fx = FC.fixture(name)
    return dict(x=fx["x"], idx=fx["idx"], centers=fx["points"], M=fx["inv_scaled_rotation"], strengths=fx["strengths"],
                min_scaling=fx["min_scaling"], density_factor=fx["density_factor"])


FIELD_N, FIELD_K, FIELD_P = (1, 255, 256, 257, 1025), (1, 15, 16, 17, 32, 33, 64), (1, 2, 300)


def shape_cases(N, K):
    """One workgroup's edge (N) against the rounds of 16 slots (K), over 1, 2 and 300 Gaussians, with and without slots outside [0, P)."""
    return [(f"{N}x{K}/{P}{'' if bad else ', every slot live'}", random_case(N, K, P, seed=3000 + N + 7 * K + P, bad_slots=bad))
            for P in FIELD_P for bad in (True, False)]


# id -> a function that returns [(label, case), ...]
FIELD_CASES = {f"{N}x{K}": (lambda N=N, K=K: shape_cases(N, K)) for N in FIELD_N for K in FIELD_K}
FIELD_CASES.update({"far": lambda: [("far", far_case())], "edge": lambda: [("edge", edge_case())]})
FIELD_CASES.update({"fixture " + name: (lambda name=name: [("fixture " + name, fixture_field_case(name))]) for name in FC.FIXTURES})


def live_slots(c):
    return int(((c["idx"] >= 0) & (c["idx"] < len(c["centers"]))).sum())


def edge_rays_case(K):
    """test_levelset_gpu.py's rays without neighbours, with a zero standard deviation and with missing slots among live ones, the
    latter in every round of 16 slots that K has."""
    c = shape_case(65, K, 21, 3, 300)
    c["idx"][3] = -1
    c["idx"][4] = 300
    c["idx"][6] = np.iinfo(np.int64).max
    c["stds"][5] = 0
    for first in range(0, K, 16):
        c["idx"][7:30:2, min(first + 5, K - 1)] = -1
        c["idx"][8:30:2, min(first + 9, K - 1)] = 300
    c["idx"][30:40, 1::2] = -1
    return c


def renormalised_case():
    c = shape_case(65, 16, 21, 3, 300)
    c["density_factor"] = 40.0
    return c


def nonfinite_march_case():
    c = shape_case(65, 16, 21, 3, 300)
    c["origins"][3, 1] = np.nan
    c["origins"][4, 0] = np.inf
    c["dirs"][5, 2] = np.nan
    c["stds"][6] = np.inf
    c["centers"] = c["centers"].copy()
    c["M"] = c["M"].copy()
    c["centers"][c["idx"][10, 2]] = np.nan
    c["M"][c["idx"][12, 0], 1, 1] = np.inf
    return c


# id -> (case, levels, S, range_size)
MARCH_CASES = {f"{n}x{K} S{S} L{L} P{P}": (lambda a=(n, K, S, L, P): (shape_case(*a), LEVELS[a[3]], a[2], 3.0)) for n, K, S, L, P in SHAPES}
MARCH_CASES.update({f"257x{K} S32 L8 P300": (lambda K=K: (shape_case(257, K, 32, 8, 300), LEVELS[8], 32, 3.0)) for K in (32, 33, 64)})
MARCH_CASES.update({f"edge rays K{K}": (lambda K=K: (edge_rays_case(K), LEVELS[3], 21, 3.0)) for K in (16, 33)})
MARCH_CASES["renormalised"] = lambda: (renormalised_case(), [0.5, 0.999], 21, 3.0)
MARCH_CASES.update({"fixture " + name: (lambda name=name: (LC.fixture_case(name), LC.fixture(name)["levels"], LC.fixture(name)["n_points_in_range"],
                                                           LC.fixture(name)["range_size"])) for name in LC.FIXTURES})


def march_range(S, range_size):
    return torch.linspace(-range_size, range_size, S).numpy()


# ---- the restatements, and wrong ones ----
def host_field(c, opacities=True, beta=True):
    d, o, b = field.field_values_host(c["x"], c["idx"], c["centers"], c["M"], c["strengths"], c["min_scaling"], c["density_factor"])
    return {"density": d, "opacities": o if opacities else None, "beta": b if beta else None}


def wrong_field(c, how):
    """field_values_host with one thing wrong.  ``expf``: the largest e moved by U + 2 steps; ``descending``: the K-sum from the last
    slot down; ``fma``: w_a's last product and sum fused (one rounding); ``slot 16``: that slot dropped."""
    x, idx, cs, M, sg, ms, valid, j = field._host_inputs(c["x"], c["idx"], c["centers"], c["M"], c["strengths"], c["min_scaling"])
    with np.errstate(all="ignore"):
        s, w, _, e, Mj = field._host_pairs(x, cs, M, j)
        if how == "fma":
            head = (Mj[..., 0, :] * s[..., 0:1] + Mj[..., 1, :] * s[..., 1:2]).astype(np.float64)
            w = (Mj[..., 2, :].astype(np.float64) * s[..., 2:3].astype(np.float64) + head).astype(F)      # (the fp64 product is exact)
            q = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
            e = np.exp(F(-0.5) * np.clip(q, 0, F(1e8))).astype(F)
        if how == "expf":
            at = np.unravel_index(np.argmax(np.where(valid, e, -1)), e.shape)
            e = e.copy()
            e[at] = CT.step(e[at], CT.U + 2)
        if how == "slot 16":
            valid = valid.copy()
            valid[:, 16] = False
        o = np.where(valid, (F(c["density_factor"]) * sg[j]) * e, F(0)).astype(F)
        d = CT.sum_asc(o[:, ::-1]) if how == "descending" else CT.sum_asc(o)
        b = CT.sum_asc(np.where(valid, ms[j], F(0))) / F(idx.shape[1])
    return {"density": d, "opacities": o, "beta": b}


def host_march(c, levels, S, range_size):
    return levelset.level_surface_host(c["origins"], c["dirs"], c["stds"], c["idx"], c["centers"], c["M"], c["strengths"], levels, S, range_size,
                                       c["density_factor"])


def wrong_t(c, got, levels):
    """The interpolation as (l - d_b) ((tau_a - tau_b) / (d_a - d_b)) + tau_b: the same real number, other roundings."""
    d, taus = got["densities"], got["taus"]
    out = dict(got, t=got["t"].copy(), points=got["points"].copy(), normals=None)
    rows = np.arange(d.shape[0])
    for l, level in enumerate(levels):
        hit, a, _ = levelset.crossing_host(d, taus, level)
        at = np.where(hit, a, 1)
        d_a, d_b, tau_a, tau_b = d[rows, at], d[rows, at - 1], taus[rows, at], taus[rows, at - 1]
        with np.errstate(all="ignore"):
            t = np.where(hit, (F(level) - d_b) * ((tau_a - tau_b) / (d_a - d_b)) + tau_b, F(0)).astype(F)
            out["t"][l] = t
            out["points"][l] = np.where(hit[:, None], c["origins"] + t[:, None] * c["dirs"], F(0)).astype(F)
    return out


# ---- the checks pass on the restatements ----
@pytest.mark.parametrize("name", list(FIELD_CASES))
def test_field_checks_pass_on_the_host_restatement(name):
    for label, c in FIELD_CASES[name]():
        stats = CT.check_field(c, host_field(c), label)
        CT.check_field(c, host_field(c, opacities=False, beta=False), label + ", density alone")
        print(label, stats)
        assert stats["density"]["elements"] == len(c["x"]) and sum(stats["steps"].values()) == live_slots(c)        # every element took part


def test_far_case_reaches_the_denormal_range():
    c = far_case()
    p = CT.Pairs(c["x"], c["idx"], c)
    denormal, zero = int((p.valid & (p.e0 > 0) & (p.e0 < TINY)).sum()), int((p.valid & (p.e0 == 0)).sum())
    print(f"far: {int(p.valid.sum())} pairs, {denormal} with a denormal e, {zero} with e == 0")
    assert denormal >= 100 and zero >= 100
    kept = field.field_values_host(c["x"], c["idx"], c["centers"], c["M"], c["strengths"])[1]
    assert ((kept > 0) & (kept < TINY)).sum() >= 100            # the contract keeps them: nothing is flushed


def test_nonfinite_field_inputs():
    c = nonfinite_field_case()
    got = host_field(c)
    stats = CT.check_field(c, got, "non-finite")
    assert np.isnan(got["density"]).any() and np.isnan(got["beta"]).any() and 0 < stats["density"]["elements"] < len(c["x"])
    got["density"][3] = F(1.0)                                   # a NaN row is still held to the sum of its own opacities
    with pytest.raises(AssertionError, match="own opacities"):
        CT.check_field(c, got, "non-finite")


@pytest.mark.parametrize("name", list(MARCH_CASES))
def test_march_checks_pass_on_the_host_restatement(name):
    c, levels, S, range_size = MARCH_CASES[name]()
    stats = CT.check_march(c, levels, march_range(S, range_size), host_march(c, levels, S, range_size), name)
    print(name, stats)
    assert stats["densities"]["elements"] == len(c["origins"]) * S
    assert stats["no_direction"] == 0 and stats["held"] == stats["hits"]          # no hit is skipped
    assert stats["hits"] > 0 or len(c["origins"]) == 1
    if name == "renormalised":
        assert (host_march(c, levels, S, range_size)["densities"] == 1).mean() > 0.3


def test_nonfinite_march_inputs():
    c, levels = nonfinite_march_case(), LEVELS[3]
    got = host_march(c, levels, 21, 3.0)
    stats = CT.check_march(c, levels, march_range(21, 3.0), got, "non-finite")
    assert np.isnan(got["densities"]).any() and 0 < stats["densities"]["elements"] < got["densities"].size and 0 < stats["held"] <= stats["hits"]
    got["hit"][1, 3] = True                                      # a ray through NaN densities is still held to the selection
    with pytest.raises(AssertionError, match="hit differs"):
        CT.check_march(c, levels, march_range(21, 3.0), got, "non-finite")


# ---- and fail on wrong ones ----
@pytest.mark.parametrize("how,match", [("expf", "window"), ("descending", "own opacities"), ("fma", "window"), ("slot 16", "window")])
def test_field_checks_fail_on_a_wrong_restatement(how, match):
    c = random_case(257, 17, 300, seed=31)
    right = host_field(c)
    same_as_host = wrong_field(c, None)
    assert all(CT.same(same_as_host[k], right[k]).all() for k in right)      # wrong_field restates the host code when nothing is wrong
    CT.check_field(c, right, "right")
    with pytest.raises(AssertionError, match=match):
        CT.check_field(c, wrong_field(c, how), how)


@pytest.mark.parametrize("how", ["expf", "fma", "slot 16"])
def test_density_enclosure_fails_without_the_opacities(how):
    """The enclosure alone, as compute_density's call and the march have it.  An e moved by U + 2 steps moves the sum by too little for
    one term among 17 unless the others are small: the case has one live slot per sample."""
    c = random_case(257, 17, 300, seed=31)
    if how == "expf":
        c["idx"][:, 1:] = -1
    if how == "fma":                      # far pairs, where the rounding of w moves e by many steps, and nothing near to hide them
        c["idx"][:, :12] = -1
    got = wrong_field(c, how)
    CT.check_field(c, dict(host_field(c), opacities=None), "right")
    with pytest.raises(AssertionError, match="density outside its enclosure"):
        CT.check_field(c, dict(got, opacities=None), how)


def test_march_checks_fail_on_a_dropped_slot_and_a_reordered_interpolation():
    c, levels, S = shape_case(257, 33, 21, 3, 300), LEVELS[3], 21
    rng = march_range(S, 3.0)
    right = host_march(c, levels, S, 3.0)
    CT.check_march(c, levels, rng, right, "right")
    dropped = dict(c, idx=c["idx"].copy())
    dropped["idx"][:, 16] = -1
    with pytest.raises(AssertionError, match="a density of the march outside its enclosure"):
        CT.check_march(c, levels, rng, host_march(dropped, levels, S, 3.0), "slot 16")
    with pytest.raises(AssertionError, match="t differs"):
        CT.check_march(c, levels, rng, wrong_t(c, right, levels), "t reordered")
    # a normal summed without slot 16, at the right points
    no_slot = dict(right, normals=right["normals"].copy())
    p = CT.Pairs(right["points"][0], dropped["idx"], c)
    with np.errstate(all="ignore"):
        o = np.where(p.valid, p.window[CT.U], F(0))
        g = np.stack([CT.sum_asc(o * p.Mw()[..., k]) for k in range(3)], 1)
        unit = -(g / np.maximum(np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]), F(1e-12))[:, None])
    no_slot["normals"][0] = np.where(right["hit"][0][:, None], unit, F(0)).astype(F)
    with pytest.raises(AssertionError, match="normal component"):
        CT.check_march(c, levels, rng, no_slot, "normals without slot 16")
