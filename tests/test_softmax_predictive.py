"""Softmax-regression scoring off the GPU: the refusals that the C ABI of csrc/predictive_softmax.hip
makes before any launch, its size function, and the fall-through of a variant to the program path."""
import numpy as np
import pytest
import torch

import numpyro_amd as numpyro
from numpyro_amd import distributions as dist
from numpyro_amd import jnp, native
from numpyro_amd.infer import log_likelihood


@pytest.mark.parametrize("n,d,k,s,ld,number", [
    (0, 3, 3, 1, 10, "n_rows >= 1 (got 0)"), (10, 65, 3, 1, 10, "dim = 65"), (10, 0, 3, 1, 10, "dim = 0"),
    (10, 3, 33, 1, 10, "num_classes = 33"), (10, 3, 1, 1, 10, "num_classes = 1"),
    (10, 3, 3, 0, 10, "num_samples = 0"), (10, 3, 3, 1, 9, "ld = 9"), (10, 3, 3, 1, 10, "NULL pointer")])
def test_shapes_outside_the_kernel_are_refused_by_name(n, d, k, s, ld, number):
    L = native.lib()
    for status in (L.nmx_softmax_loglik(0, 0, n, d, k, 0, s, 0, ld, 0), L.nmx_softmax_predict(0, n, d, k, 0, s, 7, 0, ld, 0)):
        assert status != 0 and number in L.nmx_last_error().decode()


def test_draws_past_the_counters_row_field_are_refused():
    L = native.lib()
    assert L.nmx_softmax_predict(0, (1 << 24) + 1, 3, 3, 0, 1, 7, 0, 1 << 25, 0) != 0
    assert "2^24 rows" in L.nmx_last_error().decode()


def test_the_size_function_is_zero_out_of_range():
    wb = native.lib().nmx_softmax_predictive_workspace_bytes
    assert wb(0, 3) == wb(10, 0) == wb(10, 65) == 0
    assert 0 < wb(1, 1) == wb(32, 16) < wb(33, 16) < wb(33, 17) < wb(33, 64)
    assert native.lib().nmx_softmax_predictive_pack(0, 10, 65, 0, 0) != 0
    assert "dim = 65" in native.lib().nmx_last_error().decode()


def test_a_variant_still_meets_the_program_paths_refusal():
    X, y = np.zeros((12, 3), np.float32), np.arange(12) % 4

    def model(X, y):
        W = numpyro.sample("W", dist.Normal(0.0, 1.0).expand([3, 4]))
        b = numpyro.sample("b", dist.Normal(0.0, 1.0).expand([4]))
        numpyro.sample("obs", dist.Categorical(logits=jnp.matmul(X, W) + b), obs=y)

    with pytest.raises(NotImplementedError, match="rank > 1"):
        log_likelihood(model, {"W": torch.zeros(5, 3, 4), "b": torch.zeros(5, 4)}, X, y)
