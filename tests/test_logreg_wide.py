"""Logistic regression with 65 to 1024 features off the GPU: the refusals that the C ABI makes before
any launch, the size functions, and the front end's route to the potential
(csrc/potential_logreg_wide.hip)."""
import numpy as np
import pytest

import numpyro_amd as numpyro
from numpyro_amd import distributions as dist
from numpyro_amd import jnp, native
from numpyro_amd import potentials as P
from numpyro_amd.frontend import potential_from_model


@pytest.mark.parametrize("n,d,number", [(10, 1025, "dim = 1025"), (10, 0, "dim = 0"), (10, 64, "dim = 64"),
                                        (0, 100, "n_rows = 0")])
def test_shapes_outside_the_kernel_are_refused_by_name(n, d, number):
    L = native.lib()
    ev = native.EvalBatch(num_chains=1, ldc=64)
    for status in (L.nmx_logreg_wide_pack(0, 0, n, d, 0, 0), L.nmx_logreg_wide_pe_grad(0, n, d, ev, 0, 0)):
        assert status != 0 and number in L.nmx_last_error().decode()
    assert L.nmx_logreg_wide_packed_bytes(n, d) == 0 and L.nmx_logreg_wide_workspace_bytes(n, d, 64) == 0


def test_null_pointers_are_refused():
    L = native.lib()
    ev = native.EvalBatch(num_chains=1, ldc=64)  # z, grad and pe are NULL
    for status in (L.nmx_logreg_wide_pack(0, 0, 10, 100, 0, 0), L.nmx_logreg_wide_pe_grad(0, 10, 100, ev, 0, 0)):
        assert status != 0 and "NULL" in L.nmx_last_error().decode()
    assert L.nmx_logreg_wide_workspace_bytes(10, 100, 0) == 0


def test_sizes_are_positive_and_grow():
    pb, wb = native.lib().nmx_logreg_wide_packed_bytes, native.lib().nmx_logreg_wide_workspace_bytes
    assert 0 < pb(1, 65) <= pb(33, 65) < pb(33, 129) < pb(33, 257) < pb(33, 1024) < pb(100000, 1024)
    assert 0 < wb(1, 65, 1) < wb(1, 65, 65) < wb(1, 1024, 65) <= wb(10 ** 6, 1024, 65) < wb(10 ** 6, 1024, 4096)
    assert wb(10 ** 6, 1024, 4096) <= 257 * 2 ** 20  # one workspace of the widest case; `slots` of them may exist


def test_more_than_1024_features_are_refused_naming_the_limit():
    with pytest.raises(ValueError, match="1024"):
        P.LogisticRegression(np.zeros((4, 1025), np.float32), np.zeros(4, np.float32))


def test_a_traced_100_column_model_maps_to_the_fused_potential():
    X, y = np.random.RandomState(0).randn(12, 100).astype(np.float32), (np.arange(12) % 2).astype(np.float32)

    def model(X, y):
        beta = numpyro.sample("beta", dist.Normal(0.0, 1.0).expand([100]))
        numpyro.sample("obs", dist.Bernoulli(logits=jnp.matmul(X, beta)), obs=y)

    pot = potential_from_model(model, (X, y))
    assert type(pot) is P.LogisticRegression and pot.sites == [("beta", (100,), P.REAL)] and pot.dim == 100
