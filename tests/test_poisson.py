"""Poisson regression off the GPU: the refusals the C ABI makes before any launch, and the front
end's route to potentials.PoissonRegression (csrc/potential_logreg_wide.hip, the Poisson policy)."""
import numpy as np
import pytest

import numpyro_amd as numpyro
from numpyro_amd import distributions as dist
from numpyro_amd import jnp, native, program
from numpyro_amd import potentials as P
from numpyro_amd.frontend import potential_from_model

N, D = 12, 7
X = np.random.RandomState(0).randn(N, D).astype(np.float32)
Y = np.arange(N) % 5
OFF = np.linspace(-1, 1, N).astype(np.float32)


@pytest.mark.parametrize("n,d,said", [(10, 1025, "dim = 1025"), (10, 0, "dim = 0"), (0, 100, "n_rows = 0"),
                                      (2 ** 31, 1024, "n_rows = 2147483648"), (10, 5, "NULL")])
def test_bad_shapes_and_null_pointers_are_refused_by_name(n, d, said):
    L = native.lib()
    ev = native.EvalBatch(num_chains=1, ldc=64)  # z, grad and pe are NULL
    for status in (L.nmx_poisson_pack(0, 0, 0, n, d, 0, 0), L.nmx_poisson_pe_grad(0, n, d, ev, 0, 0)):
        assert status != 0 and said in L.nmx_last_error().decode()
    if said.startswith("dim") or n == 0:
        assert L.nmx_poisson_packed_bytes(n, d) == 0 and L.nmx_poisson_workspace_bytes(n, d, 64) == 0


def test_sizes_cover_every_width_and_python_refuses_1025_features_and_bad_counts():
    pb, wb = native.lib().nmx_poisson_packed_bytes, native.lib().nmx_poisson_workspace_bytes
    assert 0 < pb(33, 1) == pb(33, 32) < pb(33, 33) == pb(33, 64) < pb(33, 65) < pb(33, 1024)
    assert wb(10, 5, 0) == 0 < wb(10, 1, 1) < wb(10, 64, 1) < wb(10, 64, 65)
    with pytest.raises(ValueError, match="1024"):
        P.PoissonRegression(np.zeros((4, 1025), np.float32), np.zeros(4, np.float32))
    for bad in (-1.0, 0.5, 2.0 ** 24):
        with pytest.raises(ValueError, match="whole numbers"):
            P.PoissonRegression(X, np.where(np.arange(N) == 3, bad, 1.0))


# name: (rate(X, b, off, s), prior scale, a further latent s, accepted by the matcher)
FORMS = {"plain": (lambda X, b, off, s: jnp.exp(jnp.matmul(X, b)), 1.0, False, True),
         "offset right": (lambda X, b, off, s: jnp.exp(jnp.matmul(X, b) + off), 1.0, False, True),
         "offset left": (lambda X, b, off, s: jnp.exp(off + jnp.matmul(X, b)), 1.0, False, True),
         "prior scale": (lambda X, b, off, s: jnp.exp(jnp.matmul(X, b)), 2.0, False, False),
         "further site": (lambda X, b, off, s: jnp.exp(jnp.matmul(X, b) + s), 1.0, True, False),
         "latent in the offset": (lambda X, b, off, s: jnp.exp(jnp.matmul(X, b) + off * b[0]), 1.0, False, False),
         "scaled rate": (lambda X, b, off, s: 2.0 * jnp.exp(jnp.matmul(X, b)), 1.0, False, False),
         "scalar offset": (lambda X, b, off, s: jnp.exp(jnp.matmul(X, b) + 0.5), 1.0, False, False)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_matcher_takes_exactly_the_fused_structure(form):
    rate, scale, extra, accepted = FORMS[form]

    def model(X, y, off):
        b = numpyro.sample("beta", dist.Normal(0.0, scale).expand([D]))
        s = numpyro.sample("s", dist.Normal(0.0, 1.0)) if extra else None
        numpyro.sample("obs", dist.Poisson(rate(X, b, off, s)), obs=y)

    if accepted:
        pot = potential_from_model(model, (X, Y, OFF))
        assert type(pot) is P.PoissonRegression and pot.sites == [("beta", (D,), P.REAL)] and pot.X_in is X
        assert (pot.o_in is None) == (form == "plain")
    else:  # a near miss compiles to a program as before
        with pytest.raises(NotImplementedError, match="no fused kernel"):
            potential_from_model(model, (X, Y, OFF))
        assert type(program.compile_model(model, (X, Y, OFF))).__name__ == "ProgramPotential"
