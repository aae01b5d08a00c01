"""Gradient-boosted tree ensembles as flat tables: scikit-learn's ``predict_proba`` for
GradientBoostingClassifier (``loss="log_loss"``) and HistGradientBoostingClassifier, restated
so the device can run it (csrc/boost.hip k_boost) and so a test can hold both against the same
arithmetic.

A boosted ensemble is not a forest with other numbers: each tree adds one scalar to one class's
raw score, the sum starts from a prior, and the result goes through a sigmoid or a softmax.

Semantics (``decision_function_numpy`` / ``predict_proba_numpy`` are the specification of the
device kernel):

* the row is cast to float32 (the engine's ML rows are fp32);
* at an inner node go left when ``(double)x[feature] <= threshold`` (threshold fp64), else
  right -- so a NaN goes right (no missing-value support);
* ``raw[k] = base[k]``; trees are stored stage-major and tree t adds the value of the leaf it
  reaches to ``raw[t % n_outputs]``, in tree order, in fp64.  For GradientBoostingClassifier
  the leaf value is ``learning_rate * value``, the fp64 product sklearn forms; a
  HistGradientBoostingClassifier's leaf values already contain the shrinkage;
* two classes (``n_outputs == 1``): ``p1 = 1 / (1 + E(-raw[0]))``, ``p0 = 1 - p1``;
* more classes: ``e[k] = E(raw[k] - max raw)``, ``p[k] = e[k] / ((e[0] + e[1]) + e[2] + ...)``
  summed in class order;
* ``E`` is fdlibm's exp as written in csrc/detmath.h (``det_exp2(x, 0.0)``), called here through
  its host build ``mv_det_exp``: host and device run the same IEEE operations, so the device's
  probabilities are these bits.

Against scikit-learn: the raw scores equal ``decision_function`` bit for bit on rows that are
float32-representable.  GradientBoostingClassifier casts ``X`` to float32 itself;
HistGradientBoostingClassifier compares in fp64, so a float64 row that rounds across a
threshold in the float32 cast follows the cast here and not there.  ``predict_proba`` differs
from sklearn's (scipy's ``expit`` / ``softmax`` on the C library's exp) by a few ulps
(DESIGN.md 7f).

Layout: ForestTables' (``feature``, ``left``, ``right`` int32 and ``threshold`` fp64 per node,
the nodes of tree t at ``tree_root[t] .. tree_root[t + 1] - 1``, root first; a leaf is a node
whose ``feature`` is ``-(leaf index + 1)``) with ``leaf_value`` fp64 ``[n_leaves]`` and
``base`` fp64 ``[n_outputs]``.
"""
from __future__ import annotations

import numpy as np

from .forest import MAX_CLASSES, MIN_CLASSES, ForestTables


def is_sklearn_boost(model) -> bool:
    """A scikit-learn GradientBoostingClassifier / HistGradientBoostingClassifier, told
    without importing sklearn when it is not loaded."""
    mod = type(model).__module__ or ""
    if not mod.startswith("sklearn."):
        return False
    from sklearn.ensemble import GradientBoostingClassifier, HistGradientBoostingClassifier

    return isinstance(model, (GradientBoostingClassifier, HistGradientBoostingClassifier))


class BoostTables:
    def __init__(self, n_features, n_classes, feature, threshold, left, right, tree_root,
                 leaf_value, base):
        self.n_features = int(n_features)
        self.n_classes = int(n_classes)
        self.feature = np.ascontiguousarray(feature, np.int32).reshape(-1)
        self.threshold = np.ascontiguousarray(threshold, np.float64).reshape(-1)
        self.left = np.ascontiguousarray(left, np.int32).reshape(-1)
        self.right = np.ascontiguousarray(right, np.int32).reshape(-1)
        self.tree_root = np.ascontiguousarray(tree_root, np.int32).reshape(-1)
        self.leaf_value = np.ascontiguousarray(leaf_value, np.float64).reshape(-1)
        self.base = np.ascontiguousarray(base, np.float64).reshape(-1)
        self.validate()

    # -- shapes
    @property
    def n_nodes(self) -> int:
        return int(self.feature.shape[0])

    @property
    def n_trees(self) -> int:
        return int(self.tree_root.shape[0])

    @property
    def n_leaves(self) -> int:
        return int(self.leaf_value.shape[0])

    @property
    def n_outputs(self) -> int:
        return int(self.base.shape[0])

    def validate(self) -> None:
        """The limits the engine checks again before any device call (mv_boost_create):
        ForestTables.validate's on the shared fields, then n_outputs is 1 exactly for two
        classes (else the class count), n_trees is a multiple of it, base and the leaf values
        are finite."""
        if not MIN_CLASSES <= self.n_classes <= MAX_CLASSES:
            raise ValueError(f"{self.n_classes} classes: the engine runs boosted ensembles of "
                             f"{MIN_CLASSES}..{MAX_CLASSES} classes")
        # the structural rules are the forest's: borrow them with a stand-in leaf table
        ForestTables(self.n_features, self.feature, self.threshold, self.left, self.right,
                     self.tree_root, np.zeros((max(self.n_leaves, 0), self.n_classes)))
        want = 1 if self.n_classes == 2 else self.n_classes
        if self.n_outputs != want:
            raise ValueError(f"base has {self.n_outputs} entries; {self.n_classes} classes take "
                             f"{want}")
        if self.n_trees % self.n_outputs:
            raise ValueError(f"{self.n_trees} trees are not a multiple of n_outputs "
                             f"{self.n_outputs} (trees are stored stage-major)")
        if not (np.isfinite(self.base).all() and np.isfinite(self.leaf_value).all()):
            raise ValueError("base and every leaf value must be finite")

    # -- constructors
    @classmethod
    def from_arrays(cls, n_features, n_classes, feature, threshold, left, right, tree_root,
                    leaf_value, base):
        """Hand-written tables (tests): the arrays of the module docstring."""
        return cls(n_features, n_classes, feature, threshold, left, right, tree_root,
                   leaf_value, base)

    @classmethod
    def from_sklearn(cls, model):
        if not is_sklearn_boost(model):
            raise ValueError(f"{type(model).__name__} is not a scikit-learn gradient-boosting "
                             "classifier")
        if getattr(model, "n_outputs_", 1) != 1 or np.ndim(model.classes_[0]) != 0:
            raise ValueError("multi-output boosted models are not supported")
        nc = int(len(model.classes_))
        if not MIN_CLASSES <= nc <= MAX_CLASSES:
            raise ValueError(f"{nc} classes: the engine runs boosted ensembles of "
                             f"{MIN_CLASSES}..{MAX_CLASSES} classes")
        if hasattr(model, "_predictors"):
            trees, base = cls._hist_trees(model)
        else:
            trees, base = cls._gb_trees(model)
        feat, thr, left, right, roots, leaves = [], [], [], [], [], []
        n0 = l0 = 0
        for f, th, lc, rc, is_leaf, val in trees:
            nl = int(is_leaf.sum())
            f = f.astype(np.int64)
            f[is_leaf] = -(l0 + np.arange(nl, dtype=np.int64)) - 1
            feat.append(f)
            thr.append(np.where(is_leaf, 0.0, th))
            left.append(np.where(is_leaf, -1, lc.astype(np.int64) + n0))
            right.append(np.where(is_leaf, -1, rc.astype(np.int64) + n0))
            leaves.append(np.ascontiguousarray(val[is_leaf], np.float64))
            roots.append(n0)
            n0 += int(f.shape[0])
            l0 += nl
        if n0 >= 2 ** 31:
            raise ValueError("node count does not fit int32")
        return cls(int(model.n_features_in_), nc, np.concatenate(feat), np.concatenate(thr),
                   np.concatenate(left), np.concatenate(right), roots, np.concatenate(leaves),
                   base)

    @staticmethod
    def _gb_trees(model):
        """GradientBoostingClassifier: estimators_[stage][k] regression trees, each scaled by
        learning_rate; the prior is the init estimator's raw prediction."""
        if model.loss not in ("log_loss", "deviance"):
            raise ValueError(f"loss={model.loss!r}: only the log-loss links raw scores to "
                             "probabilities by the sigmoid / softmax the engine computes")
        init = model.init_
        if not (isinstance(init, str) and init == "zero"):
            from sklearn.dummy import DummyClassifier

            if not isinstance(init, DummyClassifier):
                raise ValueError(f"init={type(init).__name__}: the prior must not depend on the "
                                 "row (the default init or 'zero')")
        probe = np.zeros((2, int(model.n_features_in_)), np.float32)
        probe[1] = 1.0
        raw0 = np.asarray(model._raw_predict_init(probe), np.float64)
        if not (raw0[0] == raw0[1]).all():
            raise ValueError("the init estimator's prediction depends on the row")
        lr = float(model.learning_rate)
        trees = []
        for stage in model.estimators_:
            for est in stage:
                t = est.tree_
                is_leaf = t.children_left < 0
                # learning_rate * value in fp64: the product sklearn's predict_stages forms
                val = lr * np.ascontiguousarray(t.value[:, 0, 0], np.float64)
                trees.append((t.feature, t.threshold, t.children_left, t.children_right, is_leaf,
                              val))
        return trees, raw0[0].reshape(-1)

    @staticmethod
    def _hist_trees(model):
        """HistGradientBoostingClassifier: _predictors[iteration][k].nodes records (their
        values hold the shrinkage) and _baseline_prediction."""
        trees = []
        for it in model._predictors:
            for pred in it:
                nd = pred.nodes
                is_leaf = nd["is_leaf"].astype(bool)
                if nd["is_categorical"][~is_leaf].any():
                    raise ValueError("a categorical split: the engine compares a value with a "
                                     "threshold only")
                trees.append((nd["feature_idx"], nd["num_threshold"], nd["left"], nd["right"],
                              is_leaf, nd["value"]))
        return trees, np.asarray(model._baseline_prediction, np.float64).reshape(-1)

    # -- files
    def save(self, path: str) -> str:
        """Write the ``.npz`` that ``load`` and ``load_model`` read; returns its path."""
        if not path.endswith(".npz"):
            path = path + ".npz"
        np.savez(path, boost_tables=np.int32(1), n_features=np.int32(self.n_features),
                 n_classes=np.int32(self.n_classes), feature=self.feature,
                 threshold=self.threshold, left=self.left, right=self.right,
                 tree_root=self.tree_root, leaf_value=self.leaf_value, base=self.base)
        return path

    @classmethod
    def load(cls, path: str):
        d = np.load(path, allow_pickle=False)
        if "boost_tables" not in d.files:
            raise ValueError(f"{path} does not hold boost tables")
        return cls(int(d["n_features"]), int(d["n_classes"]), d["feature"], d["threshold"],
                   d["left"], d["right"], d["tree_root"], d["leaf_value"], d["base"])

    # -- the specification
    def _raw(self, x) -> np.ndarray:
        x32 = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float32)
        if x32.shape[1] != self.n_features:
            raise ValueError(f"x has {x32.shape[1]} features, the ensemble {self.n_features}")
        xd = x32.astype(np.float64)
        n, no = xd.shape[0], self.n_outputs
        raw = np.tile(self.base, (n, 1))
        for t in range(self.n_trees):
            node = np.full(n, self.tree_root[t], np.int64)
            while True:
                f = self.feature[node]
                idx = np.nonzero(f >= 0)[0]
                if idx.size == 0:
                    break
                nd = node[idx]
                go_left = xd[idx, f[idx]] <= self.threshold[nd]
                node[idx] = np.where(go_left, self.left[nd], self.right[nd])
            raw[:, t % no] += self.leaf_value[-self.feature[node].astype(np.int64) - 1]
        return raw

    def decision_function_numpy(self, x) -> np.ndarray:
        """The raw scores, in sklearn's ``decision_function`` shape: (n,) for two classes,
        (n, n_classes) otherwise."""
        raw = self._raw(x)
        return raw[:, 0] if self.n_outputs == 1 else raw

    def predict_proba_numpy(self, x) -> np.ndarray:
        from .._native import det_exp

        raw = self._raw(x)
        with np.errstate(over="ignore", divide="ignore"):
            if self.n_outputs == 1:
                p1 = 1.0 / (1.0 + det_exp(-raw[:, 0]))
                return np.stack([1.0 - p1, p1], axis=1)
            e = det_exp(raw - raw.max(axis=1)[:, np.newaxis])
            s = e[:, 0] + e[:, 1]
            for k in range(2, self.n_classes):
                s = s + e[:, k]
            return e / s[:, np.newaxis]

    # a BoostTables is itself a classifier for Classifier(model): its host prediction
    predict_proba = predict_proba_numpy

    def boost_tables(self) -> "BoostTables":
        return self


class BoostModel:
    """What ``load_model`` returns for a boosted-ensemble file: ``predict_proba`` runs on the
    GPU (mv_forest_predict on a boost handle), as ForestModel's does."""

    def __init__(self, tables: BoostTables):
        self.tables = tables

    def boost_tables(self) -> BoostTables:
        return self.tables

    def predict_proba(self, x: np.ndarray) -> np.ndarray:
        from .._native import boost_predict_proba

        return boost_predict_proba(self.tables, x)

    def save(self, path: str) -> str:
        return self.tables.save(path)
