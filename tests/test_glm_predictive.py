"""The refusals of csrc/predictive_glm.hip's entry points and public routes without a GPU, each by name."""
import numpy as np
import pytest
import torch

from numpyro_amd import native
from numpyro_amd import potentials as P
from numpyro_amd.infer import Predictive

BERNOULLI, POISSON = native.GLM_FAMILY["bernoulli"], native.GLM_FAMILY["poisson"]


def test_the_size_function_is_zero_out_of_range():
    wb = native.lib().nmx_glm_predictive_workspace_bytes
    assert wb(10, 0, 1) == wb(10, 1025, 1) == wb(0, 3, 1) == wb(10, 3, 0) == 0
    assert 0 < wb(1, 1, 1) == wb(128, 16, 128) < wb(129, 16, 128) < wb(129, 17, 128) < wb(129, 17, 129) < wb(129, 1024, 129)


# (n_rows, dim, family, num_samples, ld, pointers given, what the message names)
@pytest.mark.parametrize("n,d,family,s,ld,p,named", [
    (10, 0, POISSON, 1, 10, 1, "dim = 0"), (10, 1025, POISSON, 1, 10, 1, "dim = 1025"),
    (0, 3, POISSON, 1, 10, 1, "n_rows"), (10, 3, 2, 1, 10, 1, "unknown family 2"),
    (10, 3, POISSON, 0, 10, 1, "num_samples = 0"), (10, 3, POISSON, 1, 9, 1, "ld = 9"),
    (10, 3, POISSON, 1, 10, 0, "NULL pointer")])
def test_bad_arguments_are_refused_by_name(n, d, family, s, ld, p, named):
    L = native.lib()
    for status in (L.nmx_glm_loglik(p, n, d, family, p, s, p, ld, 0),
                   L.nmx_glm_predict(p, n, d, family, p, s, 0, 7, p, ld, 0)):
        assert status != 0 and named in L.nmx_last_error().decode()
    if named in ("dim = 0", "dim = 1025", "n_rows", "unknown family 2", "NULL pointer"):
        assert L.nmx_glm_predictive_pack(p, p, p, n, d, family, 0, 0) != 0 and named in L.nmx_last_error().decode()


def test_bernoulli_draws_and_draws_past_the_counters_row_field_are_refused():
    L = native.lib()
    assert L.nmx_glm_predict(1, 10, 3, BERNOULLI, 1, 1, 0, 7, 1, 10, 0) != 0
    assert "family 0 has no draw kernel" in L.nmx_last_error().decode()
    assert L.nmx_glm_predict(0, (1 << 24) + 1, 3, POISSON, 0, 1, 0, 7, 0, 1 << 25, 0) != 0
    assert "2^24 rows" in L.nmx_last_error().decode()
    assert L.nmx_glm_predict(1, 10, 3, POISSON, 1, 2, (1 << 32) - 2, 7, 1, 10, 0) != 0
    assert "sample0" in L.nmx_last_error().decode()


def test_poisson_predictive_without_a_gpu_names_the_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    samples = {"coefs": torch.zeros(5, 3)}
    with pytest.raises(RuntimeError, match="needs a GPU"):
        Predictive(P.poisson_regression, samples)(0, np.zeros((12, 3), np.float32), None)
