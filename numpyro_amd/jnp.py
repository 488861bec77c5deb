"""The array functions the reference's example models call on jax.numpy (matmul, dot, tanh,
exp, log, log1p, sqrt, square, power, logaddexp, expit, sum, cumsum, logsumexp (jax.scipy.special's),
concatenate, zeros, ones, eye, shape, linalg.cholesky; indexing a vector), working on NumPy / torch
arrays and on the symbolic values of latent sites (of rank <= 2 in elementwise expressions) while
the model front end traces a model (numpyro_amd/frontend.py).  Write
``from numpyro_amd import jnp`` where a numpyro model has ``import jax.numpy as jnp``."""
from __future__ import annotations

import builtins

import numpy as np


class Sym:
    """Symbolic value in a traced model: a latent site or an operation on symbolic values.
    ``op``: "latent" (args = (name,)), or an operation name with argument values (Sym,
    numbers or arrays)."""

    __array_priority__ = 1000  # NumPy arrays defer binary operators to Sym

    def __init__(self, op, args, shape):
        self.op, self.args, self.shape = op, tuple(args), tuple(shape)

    # arithmetic builds expressions
    def _bin(self, op, other, reverse=False):
        a, b = (other, self) if reverse else (self, other)
        return Sym(op, (a, b), np.broadcast_shapes(shape_of(a), shape_of(b)))

    def __add__(self, o): return self._bin("add", o)
    def __radd__(self, o): return self._bin("add", o, True)
    def __sub__(self, o): return self._bin("sub", o)
    def __rsub__(self, o): return self._bin("sub", o, True)
    def __mul__(self, o): return self._bin("mul", o)
    def __rmul__(self, o): return self._bin("mul", o, True)
    def __truediv__(self, o): return self._bin("div", o)
    def __rtruediv__(self, o): return self._bin("div", o, True)
    def __neg__(self): return Sym("neg", (self,), self.shape)
    def __matmul__(self, o): return matmul(self, o)
    def __rmatmul__(self, o): return matmul(o, self)
    def __pow__(self, o): return self._bin("pow", o)

    __iter__ = None  # indexable, not iterable (NumPy must not unpack a Sym element by element)

    def __getitem__(self, idx):
        """Indexing on the leading axis with an int, a slice or a constant integer array
        (``alpha[group]``): Sym("getitem", (x, idx))."""
        if not self.shape:
            raise IndexError("a scalar symbolic value cannot be indexed")
        n = self.shape[0]
        if isinstance(idx, Sym) or isinstance(idx, tuple):
            raise NotImplementedError("symbolic values are indexed on the leading axis by an int, a slice or a "
                                      "constant integer array")
        if isinstance(idx, slice):
            lead = (len(range(*idx.indices(n))),)
        else:
            arr = np.asarray(idx.cpu().numpy() if hasattr(idx, "cpu") else idx)
            if arr.dtype == bool or not np.issubdtype(arr.dtype, np.integer):
                raise NotImplementedError("symbolic values are indexed by integers (no boolean masks)")
            if arr.size and (arr.min() < -n or arr.max() >= n):
                raise IndexError(f"index out of range for a symbolic value of length {n}")
            idx = int(arr) if arr.ndim == 0 else arr
            lead = arr.shape
        return Sym("getitem", (self, idx), lead + self.shape[1:])

    def __repr__(self):
        if self.op == "latent":
            return f"<{self.args[0]}>"
        return f"{self.op}({', '.join(repr(a) if isinstance(a, Sym) else type(a).__name__ for a in self.args)})"


def shape_of(x):
    if isinstance(x, Sym):
        return x.shape
    if hasattr(x, "shape"):
        return tuple(x.shape)
    return np.shape(x)


def _unary(name, fn):
    def f(x):
        if isinstance(x, Sym):
            return Sym(name, (x,), x.shape)
        return fn(np.asarray(x) if not hasattr(x, "cpu") else x.cpu().numpy())
    f.__name__ = name
    return f


tanh = _unary("tanh", np.tanh)
exp = _unary("exp", np.exp)
sqrt = _unary("sqrt", np.sqrt)
log = _unary("log", np.log)
log1p = _unary("log1p", np.log1p)
square = _unary("square", np.square)


def _expit_host(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return np.exp(-(np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))))  # exp(-softplus(-x))


# jax.scipy.special.expit (the logistic sigmoid), as examples/ucbadmit.py and proportion_test.py use it
expit = _unary("expit", _expit_host)


def sum(x, axis=None):  # noqa: A001  (jax.numpy's name)
    """Full reduction of a value of rank <= 1."""
    if isinstance(x, Sym):
        if len(x.shape) > 1 or axis not in (None, 0, -1):
            raise NotImplementedError("jnp.sum of a symbolic value is the full reduction of a vector")
        return Sym("sum", (x,), ())
    return np.sum(np.asarray(x) if not hasattr(x, "cpu") else x.cpu().numpy(), axis=axis)


def _np(x):
    return np.asarray(x) if not hasattr(x, "cpu") else x.cpu().numpy()


def cumsum(x, axis=None):
    """Cumulative sum of a value of rank <= 1."""
    if isinstance(x, Sym):
        if len(x.shape) != 1 or axis not in (None, 0, -1):
            raise NotImplementedError("jnp.cumsum of a symbolic value is the cumulative sum of a vector")
        return Sym("cumsum", (x,), x.shape)
    return np.cumsum(_np(x), axis=axis)


def logsumexp(x, axis=None):
    """jax.scipy.special.logsumexp: the full reduction of a value of rank <= 1 (a row of -inf
    gives -inf)."""
    if isinstance(x, Sym):
        if len(x.shape) > 1 or axis not in (None, 0, -1):
            raise NotImplementedError("logsumexp of a symbolic value is the full reduction of a vector")
        return Sym("logsumexp", (x,), ())
    a = np.asarray(_np(x), np.float64)
    with np.errstate(all="ignore"):
        m = np.max(a, axis=axis, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        return np.log(np.sum(np.exp(a - m), axis=axis)) + (m.reshape(()) if axis is None else np.squeeze(m, axis))


def concatenate(arrays, axis=0):
    """Concatenation of vectors (constants or symbolic values of rank 1)."""
    arrays = list(arrays)
    if builtins.any(isinstance(a, Sym) for a in arrays):
        shapes = [shape_of(a) for a in arrays]
        if builtins.any(len(s) != 1 for s in shapes) or axis not in (0, -1):
            raise NotImplementedError("jnp.concatenate with a symbolic value joins vectors (rank 1) on axis 0")
        return Sym("concatenate", arrays, (builtins.sum(s[0] for s in shapes),))
    return np.concatenate([_np(a) for a in arrays], axis=axis)


def matmul(a, b):
    if isinstance(a, Sym) or isinstance(b, Sym):
        sa, sb = shape_of(a), shape_of(b)
        out = sa[:-1] + sb[1:] if len(sb) > 1 else sa[:-1]
        return Sym("matmul", (a, b), out)
    return np.matmul(np.asarray(a), np.asarray(b))


dot = matmul


def power(x, y):
    """jax.numpy.power: elementwise x ** y (the program's pow op)."""
    if isinstance(x, Sym) or isinstance(y, Sym):
        return Sym("pow", (x, y), np.broadcast_shapes(shape_of(x), shape_of(y)))
    return np.power(_np(x), _np(y))


def logaddexp(x, y):
    """jax.numpy.logaddexp: elementwise log(exp(x) + exp(y)) (the program's logaddexp op)."""
    if isinstance(x, Sym) or isinstance(y, Sym):
        return Sym("logaddexp", (x, y), np.broadcast_shapes(shape_of(x), shape_of(y)))
    return np.logaddexp(_np(x), _np(y))


def eye(n, dtype=None):
    """float64: a constant times the identity folds on the host unrounded, as every other constant."""
    return np.eye(n)


class linalg:
    """jax.numpy.linalg: ``cholesky``."""

    @staticmethod
    def cholesky(a):
        """The lower Cholesky factor of one square matrix (its lower triangle is read)."""
        if isinstance(a, Sym):
            if len(a.shape) != 2 or a.shape[0] != a.shape[1]:
                raise NotImplementedError(f"linalg.cholesky of a symbolic value of shape {a.shape}: one square "
                                          "matrix is supported")
            return Sym("cholesky", (a,), a.shape)
        return np.linalg.cholesky(_np(a))


def zeros(shape, dtype=None):
    return np.zeros(shape, np.float32)


def ones(shape, dtype=None):
    return np.ones(shape, np.float32)


def shape(x):
    return shape_of(x)
