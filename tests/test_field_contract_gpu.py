"""gsr_field.hip on the GPU against its fp32 contract, per element and without a fitted tolerance (tests/field_contract.py): stored
opacities inside the 2-step window of expf, densities and beta bit for bit, densities without opacities and the march's densities inside
their enclosure, every ray's hit, t and point bit for bit from the kernel's own densities, normals inside the enclosure at the kernel's
own points.  The cases are those tests/test_field_contract.py passes on the numpy restatements."""
import numpy as np
import pytest

import field_contract as CT
import test_field_contract as cases
from test_field_gpu import run_op as run_field
from test_levelset_gpu import run_op as run_march

pytestmark = pytest.mark.gpu
F = np.float32


def field_outputs(c, want_opacities, want_beta):
    got = run_field(c, ups=(), grads=(), want_opacities=want_opacities, want_beta=want_beta)
    assert (got["opacities"] is None) == (not want_opacities) and (got["beta"] is None) == (not want_beta)
    return got


@pytest.mark.parametrize("name", list(cases.FIELD_CASES))
def test_field_kernel_against_its_contract(name):
    """Every combination of the two optional outputs: with the opacities stored the density is held to their sum bit for bit, without
    them to its enclosure."""
    for label, c in cases.FIELD_CASES[name]():
        for want_opacities in (True, False):
            for want_beta in (True, False):
                stats = CT.check_field(c, field_outputs(c, want_opacities, want_beta), f"{label}, opacities {want_opacities}, beta {want_beta}")
                print(f"{label}, opacities {want_opacities}, beta {want_beta}", stats)
                assert stats["density"]["elements"] == len(c["x"])                          # every element took part
                assert not want_opacities or sum(stats["steps"].values()) == cases.live_slots(c)


def test_field_kernel_keeps_denormal_opacities():
    """The far case: the contract keeps a denormal e and a denormal product, as the reference's torch path does."""
    c = cases.far_case()
    got = field_outputs(c, True, False)
    tiny = (got["opacities"] > 0) & (got["opacities"] < np.finfo(F).tiny)
    print(f"far: {int(tiny.sum())} denormal opacities stored")
    assert tiny.sum() >= 100


def test_field_kernel_on_nonfinite_inputs():
    c = cases.nonfinite_field_case()
    got = field_outputs(c, True, True)
    stats = CT.check_field(c, got, "non-finite")
    print("non-finite", stats)
    assert np.isnan(got["density"]).any() and np.isnan(got["beta"]).any() and 0 < stats["density"]["elements"] < len(c["x"])
    CT.check_field(c, field_outputs(c, False, False), "non-finite, density alone")


@pytest.mark.parametrize("name", list(cases.MARCH_CASES))
def test_march_kernel_against_its_contract(name):
    c, levels, S, range_size = cases.MARCH_CASES[name]()
    got = run_march(c, levels, S, range_size)
    stats = CT.check_march(c, levels, cases.march_range(S, range_size), got, name)
    print(name, stats)
    assert stats["densities"]["elements"] == len(c["origins"]) * S                 # every element and every ray took part
    assert stats["held"] + stats["no_direction"] == stats["hits"]
    bare = run_march(c, levels, S, range_size, want_normals=False)
    assert bare["normals"] is None and all(CT.same(bare[k], got[k]).all() for k in ("t", "points", "densities")) and np.array_equal(bare["hit"], got["hit"])


def test_march_kernel_on_nonfinite_inputs():
    c, levels = cases.nonfinite_march_case(), cases.LEVELS[3]
    got = run_march(c, levels, 21, 3.0)
    stats = CT.check_march(c, levels, cases.march_range(21, 3.0), got, "non-finite")
    print("non-finite", stats)
    assert np.isnan(got["densities"]).any() and 0 < stats["densities"]["elements"] < got["densities"].size and 0 < stats["held"] <= stats["hits"]
