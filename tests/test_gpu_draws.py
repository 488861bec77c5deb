"""The draw ops of the predictive program kernel against their exact distributions: the table,
statistics, independence checks and ranges of tests/draw_cases.py on device draws.  The device
draws are compared with the distribution here; tests/test_gpu_predictive_program.py and
tests/test_gpu_bounded.py compare them with the host interpreter."""
import functools

import numpy as np
import pytest

import draw_cases as DC
from numpyro_amd.infer import Predictive

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _device_draws(name, seed):
    """One Predictive call per model and seed; {site: draws} as NumPy arrays."""
    if name == "dirichlet":
        fn, S = DC.dirichlet_model, DC.SAMPLES * DC.ELEMENTS
    else:
        fn, S = (DC.limit_model if name == "limit" else DC.model(name)), DC.SAMPLES
    out = {k: v.cpu().numpy() for k, v in Predictive(fn, num_samples=S)(seed).items()}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _floor():
    """The threshold below which a float32 gamma draw is exactly 0 on this device: 2^-150 where
    denormals are kept, 2^-126 where they are flushed."""
    kept = [DC.zero_share(_device_draws("gamma", DC.SEEDS[0])[f"gamma_{DC._num(a)}"], a,
                          [DC.DENORMALS_KEPT, DC.DENORMALS_FLUSHED]) for a in (0.02, 0.05)]
    assert kept[0] == kept[1], kept
    print("the device", "keeps" if kept[0] == DC.DENORMALS_KEPT else "flushes", "float32 denormals in the gamma boost")
    return kept[0]


def test_gamma_underflows_to_zero_as_often_as_the_law_says(device):
    x = _device_draws("gamma", DC.SEEDS[0])["gamma_0p02"]
    assert x.dtype == np.float32 and x.shape == (DC.SAMPLES, DC.ELEMENTS)
    assert _floor() in (DC.DENORMALS_KEPT, DC.DENORMALS_FLUSHED)


@pytest.mark.parametrize("family", DC.FAMILIES)
def test_device_draws_follow_their_distributions(device, family):
    DC.check_family(family, _device_draws, lambda model, seed: _floor())


def test_device_dirichlet_marginals_are_beta(device):
    DC.check_dirichlet(_device_draws)


def test_device_sites_are_independent_and_inside_their_ranges(device):
    draws = _device_draws("base", DC.SEEDS[0])
    DC.check_independence(draws)
    DC.check_ranges(draws)
    for name in DC.MODELS:
        DC.check_integer_sites(_device_draws(name, DC.SEEDS[0]), device=True)


def test_beta_and_studentt_far_below_one_keep_what_the_docs_promise(device):
    DC.limit_shares(_device_draws("limit", DC.SEEDS[0]))
