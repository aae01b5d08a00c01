"""Tree ensembles as flat tables: scikit-learn's ``predict_proba`` for RandomForestClassifier,
ExtraTreesClassifier and a single DecisionTreeClassifier, restated so the device can run it
(csrc/forest.hip k_forest) and so a test can hold both against the same arithmetic.

Semantics (``predict_proba_numpy`` is the specification of the device kernel):

* the row is cast to float32, as sklearn casts ``X``;
* at an inner node go left when ``(double)x[feature] <= threshold`` (threshold fp64), else
  right -- so a NaN goes right (no missing-value support);
* a leaf's row is ``value[leaf] / normalizer``, ``normalizer = value[leaf].sum()`` or 1 where
  that sum is 0, computed once here in fp64;
* the forest's probability is the fp64 sum of the trees' leaf rows in ``estimators_`` order,
  starting from 0.0, divided by the number of trees.

Layout: ``feature``, ``left``, ``right`` int32 and ``threshold`` fp64 per node, the nodes of
tree t at ``tree_root[t] .. tree_root[t + 1] - 1`` (its root first); a leaf is a node whose
``feature`` is ``-(leaf index + 1)``, its row ``leaf_value[leaf index]``.
"""
from __future__ import annotations

import numpy as np

MIN_CLASSES, MAX_CLASSES = 2, 8


def is_sklearn_trees(model) -> bool:
    """A fitted sklearn RandomForestClassifier / ExtraTreesClassifier / DecisionTreeClassifier
    (or ExtraTreeClassifier), told without importing sklearn when it is not loaded."""
    mod = type(model).__module__ or ""
    if not mod.startswith("sklearn."):
        return False
    from sklearn.ensemble import ExtraTreesClassifier, RandomForestClassifier
    from sklearn.tree import DecisionTreeClassifier

    return isinstance(model, (RandomForestClassifier, ExtraTreesClassifier,
                              DecisionTreeClassifier))


class ForestTables:
    def __init__(self, n_features, feature, threshold, left, right, tree_root, leaf_value):
        self.n_features = int(n_features)
        self.feature = np.ascontiguousarray(feature, np.int32).reshape(-1)
        self.threshold = np.ascontiguousarray(threshold, np.float64).reshape(-1)
        self.left = np.ascontiguousarray(left, np.int32).reshape(-1)
        self.right = np.ascontiguousarray(right, np.int32).reshape(-1)
        self.tree_root = np.ascontiguousarray(tree_root, np.int32).reshape(-1)
        self.leaf_value = np.ascontiguousarray(leaf_value, np.float64)
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
    def n_classes(self) -> int:
        return int(self.leaf_value.shape[1])

    def validate(self) -> None:
        """The limits the engine checks again before any device call (mv_forest_create):
        2..8 classes, at least one tree, features in [0, D), every child inside its own tree
        and after its parent (so no walk can cycle), node count within int32."""
        if self.leaf_value.ndim != 2:
            raise ValueError("leaf_value must be (n_leaves, n_classes)")
        if not MIN_CLASSES <= self.n_classes <= MAX_CLASSES:
            raise ValueError(f"{self.n_classes} classes: the engine runs forests of "
                             f"{MIN_CLASSES}..{MAX_CLASSES} classes")
        if self.n_trees < 1:
            raise ValueError("a forest needs at least one tree")
        if self.n_features < 1:
            raise ValueError("n_features must be positive")
        n = self.n_nodes
        if n >= 2 ** 31:
            raise ValueError("node count does not fit int32")
        if not (self.threshold.shape[0] == self.left.shape[0] == self.right.shape[0] == n):
            raise ValueError("feature, threshold, left and right must have one entry per node")
        roots = self.tree_root.astype(np.int64)
        if roots[0] != 0 or (np.diff(roots) <= 0).any() or roots[-1] >= n:
            raise ValueError("tree_root must start at 0 and ascend inside the node array")
        end = np.append(roots[1:], n)
        tree_end = np.repeat(end, end - roots)  # per node: one past its tree's last node
        idx = np.arange(n, dtype=np.int64)
        leaf = self.feature < 0
        inner = ~leaf
        if (self.feature[inner] >= self.n_features).any():
            raise ValueError("a split feature lies outside [0, n_features)")
        li = -(self.feature[leaf].astype(np.int64)) - 1
        if (li >= self.n_leaves).any():
            raise ValueError("a leaf index lies outside leaf_value")
        for child in (self.left, self.right):
            c = child[inner].astype(np.int64)
            if (c <= idx[inner]).any():
                raise ValueError("a child index is not greater than its parent's")
            if (c >= tree_end[inner]).any():
                raise ValueError("a child index lies outside its tree")
        kids = np.concatenate([self.left[inner], self.right[inner]])
        if np.unique(kids).size != kids.size:
            raise ValueError("a node has two parents")

    # -- constructors
    @classmethod
    def from_arrays(cls, n_features, feature, threshold, left, right, tree_root, leaf_value):
        """Hand-written tables (tests): the arrays of the module docstring."""
        return cls(n_features, feature, threshold, left, right, tree_root, leaf_value)

    @classmethod
    def from_sklearn(cls, model):
        if not is_sklearn_trees(model):
            raise ValueError(f"{type(model).__name__} is not a scikit-learn forest or tree "
                             "classifier")
        if getattr(model, "n_outputs_", 1) != 1:
            raise ValueError("multi-output forests are not supported")
        trees = [e.tree_ for e in model.estimators_] if hasattr(model, "estimators_") \
            else [model.tree_]
        nc = int(model.n_classes_)
        feat, thr, left, right, roots, leaves = [], [], [], [], [], []
        n0 = l0 = 0
        for t in trees:
            is_leaf = t.children_left < 0
            f = t.feature.astype(np.int64)
            f[is_leaf] = -(l0 + np.arange(int(is_leaf.sum()), dtype=np.int64)) - 1
            v = np.ascontiguousarray(t.value[is_leaf][:, 0, :nc], np.float64)
            norm = v.sum(axis=1)[:, np.newaxis]
            norm[norm == 0.0] = 1.0
            leaves.append(v / norm)
            feat.append(f)
            thr.append(np.where(is_leaf, 0.0, t.threshold))
            left.append(np.where(is_leaf, -1, t.children_left.astype(np.int64) + n0))
            right.append(np.where(is_leaf, -1, t.children_right.astype(np.int64) + n0))
            roots.append(n0)
            n0 += int(t.node_count)
            l0 += int(is_leaf.sum())
        if n0 >= 2 ** 31:
            raise ValueError("node count does not fit int32")
        return cls(int(model.n_features_in_), np.concatenate(feat), np.concatenate(thr),
                   np.concatenate(left), np.concatenate(right), roots, np.concatenate(leaves))

    # -- files
    def save(self, path: str) -> str:
        """Write the ``.npz`` that ``load`` and ``load_model`` read; returns its path."""
        if not path.endswith(".npz"):
            path = path + ".npz"
        np.savez(path, forest_tables=np.int32(1), n_features=np.int32(self.n_features),
                 feature=self.feature, threshold=self.threshold, left=self.left,
                 right=self.right, tree_root=self.tree_root, leaf_value=self.leaf_value)
        return path

    @classmethod
    def load(cls, path: str):
        d = np.load(path, allow_pickle=False)
        if "forest_tables" not in d.files:
            raise ValueError(f"{path} does not hold forest tables")
        return cls(int(d["n_features"]), d["feature"], d["threshold"], d["left"], d["right"],
                   d["tree_root"], d["leaf_value"])

    # -- the specification
    def predict_proba_numpy(self, x) -> np.ndarray:
        x32 = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float32)
        if x32.shape[1] != self.n_features:
            raise ValueError(f"x has {x32.shape[1]} features, the forest {self.n_features}")
        xd = x32.astype(np.float64)
        n = xd.shape[0]
        acc = np.zeros((n, self.n_classes), np.float64)
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
            acc += self.leaf_value[-self.feature[node].astype(np.int64) - 1]
        acc /= self.n_trees
        return acc

    # a ForestTables is itself a classifier for Classifier(model): its host prediction
    predict_proba = predict_proba_numpy

    def forest_tables(self) -> "ForestTables":
        return self


class ForestModel:
    """What ``load_model`` returns for a forest file: ``predict_proba`` runs on the GPU
    (mv_forest_predict), as DenseMLPModel's does."""

    def __init__(self, tables: ForestTables):
        self.tables = tables

    def forest_tables(self) -> ForestTables:
        return self.tables

    def predict_proba(self, x: np.ndarray) -> np.ndarray:
        from .._native import forest_predict_proba

        return forest_predict_proba(self.tables, x)

    def save(self, path: str) -> str:
        return self.tables.save(path)
