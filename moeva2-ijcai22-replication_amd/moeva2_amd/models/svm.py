"""Kernel machines and logistic regression as flat tables: scikit-learn's ``predict_proba`` for
``SVC`` / ``NuSVC`` (``probability=True``, two classes; linear, poly and rbf kernels) and
``LogisticRegression`` (2..8 classes), restated so the device can run it (csrc/svm.hip k_svm)
and so a test can hold both against the same arithmetic.

Semantics (``predict_proba_numpy`` is the specification of the device kernel):

* the row is cast to float32 and back to float64 (the engine's ML rows are fp32);
* per vector v, the feature sum ``s_v`` starts at 0 and takes one *fused* multiply-add per
  feature, in ascending feature order: ``s = fma(x_j, v_j, s)`` (linear, poly) or
  ``d = x_j - v_j; s = fma(d, d, s)`` (rbf).  numpy has no fma, so the sums come from
  ``mv_svm_sums``, the host build of the inline function the kernel calls (csrc/svm.h
  ``svm_term``), as ``E`` below comes from ``mv_det_exp``;
* ``K_v = s_v`` (linear); ``powi(gamma * s_v + coef0, degree)`` (poly: libsvm's
  square-and-multiply over the bits of the degree, every product rounded); ``E(-(gamma * s_v))``
  (rbf);
* ``dec[o] = 0``, then over the vectors in ascending order ``dec[o] = dec[o] + coef[o][v] * K_v``
  (a rounded product, then a rounded sum), then ``dec[o] = dec[o] + intercept[o]``.  Without
  ``coef`` (logistic regression: the vectors are ``coef_``'s rows) ``dec[o] = K_o +
  intercept[o]``;
* link ``platt`` (SVC / NuSVC): libsvm's own decision value is ``-dec[0]``;
  ``f = (-dec[0]) * probA + probB``; ``s = e / (1 + e)`` with ``e = E(-f)`` when ``f >= 0``,
  else ``1 / (1 + E(f))``; ``s`` is clipped as libsvm writes it, ``s = s if s > 1e-7 else 1e-7``
  then ``s = s if s < 1 - 1e-7 else 1 - 1e-7`` (a NaN becomes 1e-7); then libsvm's
  ``multiclass_probability`` for two classes on ``r01 = s``, ``r10 = 1 - s`` (``couple2``: from
  p = (0.5, 0.5), eps = 0.005 / 2, at most 100 iterations, every operation in libsvm's order);
* link ``sigmoid`` (logistic regression, two classes): ``p1 = 1 / (1 + E(-dec[0]))``,
  ``p0 = 1 - p1``;
* link ``softmax`` (3..8 classes): ``e[k] = E(dec[k] - max dec)``,
  ``p[k] = e[k] / ((e[0] + e[1]) + e[2] + ...)`` in class order;
* ``E`` is fdlibm's exp as written in csrc/detmath.h (``det_exp2(x, 0.0)``).

None of these orders depends on the number of rows or on how the device launches them.

Against scikit-learn 1.7.2 the probabilities differ in the last bits (libsvm and BLAS sum in
another order and without fma, and the C library's exp is another exp): DESIGN.md 7g.
"""
from __future__ import annotations

import numpy as np

MIN_CLASSES, MAX_CLASSES = 2, 8
MAX_ENTRIES = 1 << 24  # n_vec * n_features (csrc/svm.h SVM_MAX_ENTRIES): 128 MiB of fp64
MAX_DEGREE = 64
KERNELS = ("linear", "poly", "rbf")          # mv_svm_desc.kernel
LINKS = ("platt", "sigmoid", "softmax")      # mv_svm_desc.link
_LO, _HI = 1e-7, 1 - 1e-7


def is_sklearn_svm(model) -> bool:
    """A scikit-learn SVC / NuSVC / LogisticRegression, told without importing sklearn when it
    is not loaded."""
    mod = type(model).__module__ or ""
    if not mod.startswith("sklearn."):
        return False
    from sklearn.linear_model import LogisticRegression
    from sklearn.svm import SVC, NuSVC

    return isinstance(model, (SVC, NuSVC, LogisticRegression))


def powi(base: np.ndarray, times: int) -> np.ndarray:
    """libsvm's powi."""
    tmp = np.array(base, np.float64)
    ret = np.ones_like(tmp)
    t = int(times)
    while t > 0:
        if t % 2 == 1:
            ret = ret * tmp
        tmp = tmp * tmp
        t //= 2
    return ret


def couple2(r01, return_iters=False):
    """libsvm's multiclass_probability for k = 2, elementwise on r01 (r10 = 1 - r01): the
    probabilities ``[n][2]`` (and the iterations each element took)."""
    r01 = np.atleast_1d(np.asarray(r01, np.float64))
    r10 = 1.0 - r01
    q00, q01, q11, eps = r10 * r10, (-r10) * r01, r01 * r01, 0.005 / 2
    p0 = np.full(r01.shape, 0.5)
    p1 = np.full(r01.shape, 0.5)
    iters = np.zeros(r01.shape, np.int64)
    live = np.ones(r01.shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(100):
            qp0 = q00 * p0 + q01 * p1
            qp1 = q01 * p0 + q11 * p1
            pqp = p0 * qp0 + p1 * qp1
            e0, e1 = np.abs(qp0 - pqp), np.abs(qp1 - pqp)
            err = np.where(e0 > 0.0, e0, 0.0)
            err = np.where(e1 > err, e1, err)
            live = live & ~(err < eps)
            if not live.any():
                break
            iters = iters + live
            diff = (-qp0 + pqp) / q00
            n0 = p0 + diff
            pqp = (pqp + diff * (diff * q00 + 2 * qp0)) / (1 + diff) / (1 + diff)
            n0 = n0 / (1 + diff)
            qp1 = (qp1 + diff * q01) / (1 + diff)
            n1 = p1 / (1 + diff)
            diff = (-qp1 + pqp) / q11
            n1 = n1 + diff
            n0 = n0 / (1 + diff)
            n1 = n1 / (1 + diff)
            p0 = np.where(live, n0, p0)
            p1 = np.where(live, n1, p1)
    p = np.stack([p0, p1], axis=-1)
    return (p, iters) if return_iters else p


class SvmTables:
    def __init__(self, n_features, n_classes, vectors, coef, intercept, kernel="linear",
                 gamma=0.0, coef0=0.0, degree=0, link="platt", probA=0.0, probB=0.0):
        self.n_features = int(n_features)
        self.n_classes = int(n_classes)
        if hasattr(vectors, "toarray") or (coef is not None and hasattr(coef, "toarray")):
            raise ValueError("sparse vectors: the engine takes dense tables")
        self.vectors = np.ascontiguousarray(vectors, np.float64)
        self.coef = None if coef is None else np.ascontiguousarray(coef, np.float64)
        self.intercept = np.ascontiguousarray(intercept, np.float64).reshape(-1)
        if callable(kernel) or kernel not in KERNELS:
            raise ValueError(f"kernel={kernel!r}: the engine runs {', '.join(KERNELS)}")
        self.kernel = kernel
        if link not in LINKS:
            raise ValueError(f"link={link!r}: one of {', '.join(LINKS)}")
        self.link = link
        if isinstance(degree, bool) or float(degree) != int(degree) or int(degree) < 0:
            raise ValueError(f"degree={degree!r}: libsvm's powi takes a non-negative integer")
        self.degree = int(degree)
        self.gamma, self.coef0 = float(gamma), float(coef0)
        self.probA, self.probB = float(probA), float(probB)
        self.validate()

    # -- shapes
    @property
    def n_vec(self) -> int:
        return int(self.vectors.shape[0])

    @property
    def n_out(self) -> int:
        return int(self.intercept.shape[0])

    def validate(self) -> None:
        """The limits the engine checks again before any device call (api.cpp svm_check)."""
        if self.vectors.ndim != 2 or self.vectors.shape[1] != self.n_features or \
                self.n_features < 1:
            raise ValueError(f"vectors {self.vectors.shape}: expected [n_vec][{self.n_features}]")
        if self.n_vec < 1:
            raise ValueError("n_vec < 1: no vector")
        if self.n_vec * self.n_features > MAX_ENTRIES:
            raise ValueError(f"n_vec * n_features = {self.n_vec * self.n_features} above "
                             f"{MAX_ENTRIES}")
        if not MIN_CLASSES <= self.n_classes <= MAX_CLASSES:
            raise ValueError(f"{self.n_classes} classes: the engine runs {MIN_CLASSES}.."
                             f"{MAX_CLASSES}")
        if self.link == "softmax":
            if self.n_classes < 3 or self.n_out != self.n_classes:
                raise ValueError("softmax takes 3..8 classes and one decision per class")
        elif self.n_classes != 2 or self.n_out != 1:
            raise ValueError(f"link {self.link} takes two classes and one decision "
                             f"(got {self.n_classes} classes, {self.n_out} decisions)")
        if self.coef is None:
            if self.n_vec != self.n_out:
                raise ValueError("without coef the vectors are the decisions' rows: "
                                 f"n_vec {self.n_vec} != n_out {self.n_out}")
        elif self.coef.shape != (self.n_out, self.n_vec):
            raise ValueError(f"coef {self.coef.shape}: expected ({self.n_out}, {self.n_vec})")
        if self.degree > MAX_DEGREE:
            raise ValueError(f"degree {self.degree} above {MAX_DEGREE}")
        arrays = [self.vectors, self.intercept,
                  np.array([self.gamma, self.coef0, self.probA, self.probB])]
        if self.coef is not None:
            arrays.append(self.coef)
        if not all(np.isfinite(a).all() for a in arrays):
            raise ValueError("every table entry and parameter must be finite")

    # -- constructors
    @classmethod
    def from_arrays(cls, n_features, n_classes, vectors, coef, intercept, kernel="linear",
                    gamma=0.0, coef0=0.0, degree=0, link="platt", probA=0.0, probB=0.0):
        """Hand-written tables (tests): the arrays of the module docstring."""
        return cls(n_features, n_classes, vectors, coef, intercept, kernel, gamma, coef0, degree,
                   link, probA, probB)

    @classmethod
    def from_sklearn(cls, model):
        if not is_sklearn_svm(model):
            raise ValueError(f"{type(model).__name__} is not a scikit-learn SVC, NuSVC or "
                             "LogisticRegression")
        nc = int(len(model.classes_))
        if not MIN_CLASSES <= nc <= MAX_CLASSES:
            raise ValueError(f"{nc} classes: the engine runs {MIN_CLASSES}..{MAX_CLASSES}")
        if hasattr(model, "support_vectors_"):
            return cls._from_svc(model, nc)
        return cls._from_logreg(model, nc)

    @classmethod
    def _from_svc(cls, m, nc):
        if callable(m.kernel) or m.kernel not in KERNELS:
            raise ValueError(f"kernel={m.kernel!r}: the engine runs {', '.join(KERNELS)}")
        if not m.probability:
            raise ValueError("probability=False: the model has no predict_proba")
        if nc != 2:
            raise ValueError(f"an SVC of {nc} classes: the engine couples two classes only")
        if getattr(m, "_sparse", False) or hasattr(m.support_vectors_, "toarray"):
            raise ValueError("sparse support vectors: the engine takes dense tables")
        # decision_function = dual_coef_ . K + intercept_ ; libsvm's own value is its negation
        return cls(int(m.support_vectors_.shape[1]), nc, m.support_vectors_, m.dual_coef_,
                   m.intercept_, m.kernel, m._gamma, m.coef0, m.degree, "platt",
                   float(m.probA_[0]), float(m.probB_[0]))

    @classmethod
    def _from_logreg(cls, m, nc):
        mc = getattr(m, "multi_class", "deprecated")
        ovr = mc in ("ovr", "warn") or (mc in ("auto", "deprecated")
                                        and (nc <= 2 or m.solver == "liblinear"))
        if ovr and nc > 2:
            raise ValueError("a one-vs-rest LogisticRegression of more than two classes "
                             "normalises per-class sigmoids: not the softmax the engine computes")
        if not ovr and nc == 2:
            raise ValueError("a multinomial LogisticRegression of two classes takes the softmax "
                             "of (-d, d): not the sigmoid the engine computes")
        if hasattr(m.coef_, "toarray"):
            raise ValueError("sparse coefficients: the engine takes dense tables")
        return cls(int(m.coef_.shape[1]), nc, m.coef_, None, m.intercept_, "linear",
                   link="sigmoid" if nc == 2 else "softmax")

    # -- files
    def save(self, path: str) -> str:
        """Write the ``.npz`` that ``load`` and ``load_model`` read; returns its path."""
        if not path.endswith(".npz"):
            path = path + ".npz"
        np.savez(path, svm_tables=np.int32(1), n_features=np.int32(self.n_features),
                 n_classes=np.int32(self.n_classes), vectors=self.vectors,
                 has_coef=np.int32(self.coef is not None),
                 coef=self.coef if self.coef is not None else np.zeros((0, 0)),
                 intercept=self.intercept, kernel=np.int32(KERNELS.index(self.kernel)),
                 link=np.int32(LINKS.index(self.link)), degree=np.int32(self.degree),
                 params=np.array([self.gamma, self.coef0, self.probA, self.probB]))
        return path

    @classmethod
    def load(cls, path: str):
        d = np.load(path, allow_pickle=False)
        if "svm_tables" not in d.files:
            raise ValueError(f"{path} does not hold svm tables")
        g, c0, pa, pb = (float(v) for v in d["params"])
        return cls(int(d["n_features"]), int(d["n_classes"]), d["vectors"],
                   d["coef"] if int(d["has_coef"]) else None, d["intercept"],
                   KERNELS[int(d["kernel"])], g, c0, int(d["degree"]), LINKS[int(d["link"])],
                   pa, pb)

    # -- the specification
    def kernel_values_numpy(self, x) -> np.ndarray:
        """K(x_i, v) ``[n][n_vec]``."""
        from .._native import det_exp, svm_sums

        x32 = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float32)
        if x32.shape[1] != self.n_features:
            raise ValueError(f"x has {x32.shape[1]} features, the model {self.n_features}")
        s = svm_sums(x32.astype(np.float64), self.vectors, self.kernel == "rbf")
        with np.errstate(all="ignore"):
            if self.kernel == "rbf":
                return det_exp(-(self.gamma * s))
            if self.kernel == "poly":
                return powi(self.gamma * s + self.coef0, self.degree)
        return s

    def decision_function_numpy(self, x) -> np.ndarray:
        """The decisions, in sklearn's ``decision_function`` shape: (n,) for two classes,
        (n, n_classes) otherwise."""
        k = self.kernel_values_numpy(x)
        with np.errstate(all="ignore"):
            if self.coef is None:
                dec = k + self.intercept[np.newaxis, :]
            else:
                dec = np.zeros((k.shape[0], self.n_out))
                for v in range(self.n_vec):  # vector order, product then sum
                    dec = dec + self.coef[np.newaxis, :, v] * k[:, v:v + 1]
                dec = dec + self.intercept[np.newaxis, :]
        return dec[:, 0] if self.n_out == 1 else dec

    def predict_proba_numpy(self, x) -> np.ndarray:
        from .._native import det_exp

        dec = self.decision_function_numpy(x)
        with np.errstate(all="ignore"):
            if self.link == "platt":
                f = (-dec) * self.probA + self.probB
                pos = f >= 0
                e = det_exp(np.where(pos, -f, f))
                s = np.where(pos, e / (1.0 + e), 1.0 / (1.0 + e))
                s = np.where(s > _LO, s, _LO)
                s = np.where(s < _HI, s, _HI)
                return couple2(s)
            if self.link == "sigmoid":
                p1 = 1.0 / (1.0 + det_exp(-dec))
                return np.stack([1.0 - p1, p1], axis=1)
            e = det_exp(dec - dec.max(axis=1)[:, np.newaxis])
            s = e[:, 0] + e[:, 1]
            for k in range(2, self.n_classes):
                s = s + e[:, k]
            return e / s[:, np.newaxis]

    # an SvmTables is itself a classifier for Classifier(model): its host prediction
    predict_proba = predict_proba_numpy

    def svm_tables(self) -> "SvmTables":
        return self


class SvmModel:
    """What ``load_model`` returns for such a file: ``predict_proba`` runs on the GPU
    (mv_forest_predict on an svm handle), as BoostModel's does."""

    def __init__(self, tables: SvmTables):
        self.tables = tables

    def svm_tables(self) -> SvmTables:
        return self.tables

    def predict_proba(self, x: np.ndarray) -> np.ndarray:
        from .._native import svm_predict_proba

        return svm_predict_proba(self.tables, x)

    def save(self, path: str) -> str:
        return self.tables.save(path)
