"""The draw ops of predictive programs against their exact distributions, without a GPU: the
table of tests/draw_cases.py on the host interpreter in float64 and in float32.  The float32 run
is the arithmetic the device uses, so a formula that is right in exact arithmetic and wrong in
float32 (a cancellation at a large rate or count) shows here."""
import numpy as np
import pytest

import draw_cases as DC

DTYPES = [np.float64, np.float32]


def _draws(dtype):
    return lambda model, seed: DC.host_draws(model, seed, dtype)


def _floor(dtype):
    return lambda model, seed: DC.host_floor(model, seed, dtype)


def test_the_table_covers_every_draw_op_and_every_sampler():
    from numpyro_amd import native
    from numpyro_amd.predictive_program import _DRAW, compile_predictive

    ops, classes = set(), set()
    for name in DC.MODELS:
        prog = compile_predictive(DC.model(name), (), {}, [])
        ops |= {n for n in prog.op_names() if n.startswith("draw_")}
        classes |= {type(c.make()) for c in DC.CASES if c.model == name}
    assert ops == set(native.DRAW_OPCODES)
    assert classes | {type(DC.dist.Dirichlet(np.ones(2)))} == set(_DRAW)
    rates = [c.law.args[0] for c in DC.CASES if c.family == "poisson"]
    assert any(r < native.POISSON_PTRS_RATE for r in rates) and native.POISSON_PTRS_RATE in rates
    assert DC.MAX_RATE >= 2.0 ** 20 and DC.MAX_RATE / 2 in rates and max(rates) == DC.BELOW_MAX_RATE < DC.MAX_RATE


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("family", DC.FAMILIES)
def test_host_draws_follow_their_distributions(family, dtype):
    DC.check_family(family, _draws(dtype), _floor(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_host_dirichlet_marginals_are_beta(dtype):
    DC.check_dirichlet(_draws(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_host_sites_are_independent_and_inside_their_ranges(dtype):
    draws = DC.host_draws("base", DC.SEEDS[0], dtype)
    DC.check_independence(draws)
    DC.check_ranges(draws)
    for name in DC.MODELS:
        DC.check_integer_sites(DC.host_draws(name, DC.SEEDS[0], dtype), device=False)


@pytest.mark.parametrize("a", [0.02, 0.05])
def test_float32_gamma_underflows_to_zero_as_often_as_the_law_says(a):
    x = DC.host_draws("gamma", DC.SEEDS[0], np.float32)[f"gamma_{DC._num(a)}"]
    assert x.dtype == np.float32
    DC.zero_share(x, a, [DC.host_floor("gamma", DC.SEEDS[0], np.float32)])
    assert not (DC.host_draws("gamma", DC.SEEDS[0], np.float64)[f"gamma_{DC._num(a)}"] == 0).any()


def test_float32_beta_and_studentt_far_below_one_keep_what_the_docs_promise():
    DC.limit_shares(DC.host_draws("limit", DC.SEEDS[0], np.float32))
