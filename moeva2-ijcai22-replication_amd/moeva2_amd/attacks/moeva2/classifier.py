"""Classifier wrapper (mirror of src/attacks/moeva2/classifier.py) + the Dense-MLP model the
engine runs on MFMA.

``load_model(path)`` replaces ``tf.keras.models.load_model`` (src/utils/in_out.py:111-127)
for the Keras Sequential(Dense...) classifiers shipped with the reference: a SavedModel
directory is read with the tensor-bundle reader (no TensorFlow), an ``.npz`` produced by
tools/import_reference_data.py is read directly.

Engine extension: tree ensembles.  A ``.joblib`` file holding a fitted scikit-learn
RandomForestClassifier / ExtraTreesClassifier / DecisionTreeClassifier, or the ``.npz`` of a
``models.forest.ForestTables``, loads as a ``ForestModel`` whose trees run on the device.
A ``.joblib`` holding a GradientBoostingClassifier (log-loss) / HistGradientBoostingClassifier,
or the ``.npz`` of a ``models.boost.BoostTables``, loads as a ``BoostModel`` in the same way.
A ``.joblib`` holding an SVC / NuSVC (``probability=True``, two classes) or a
LogisticRegression, or the ``.npz`` of a ``models.svm.SvmTables``, loads as an ``SvmModel``.
"""
import os

import numpy as np

from ...io.tf_bundle import DenseMLP, load_dense_mlp
from ...models.boost import BoostModel, BoostTables, is_sklearn_boost
from ...models.forest import ForestModel, ForestTables, is_sklearn_trees
from ...models.svm import SvmModel, SvmTables, is_sklearn_svm


class DenseMLPModel:
    """Keras-equivalent Dense(relu)...Dense(softmax) model; predict_proba runs on the GPU."""

    def __init__(self, mlp: DenseMLP):
        if any(a != "relu" for a in mlp.activations[:-1]) or mlp.activations[-1] != "softmax":
            raise ValueError(f"unsupported activations {mlp.activations}")
        self.mlp = mlp

    def dense_weights(self) -> DenseMLP:
        return self.mlp

    def predict_proba(self, x: np.ndarray) -> np.ndarray:
        from ..._native import predict_proba

        return predict_proba(self.mlp, x)

    def save(self, path: str) -> str:
        """Write the ``.npz`` that ``load_model`` reads (W{i}, b{i}, activations); returns
        the file's path (``.npz`` is appended to a path without it)."""
        if not path.endswith(".npz"):
            path = path + ".npz"
        arrays = {"activations": np.array(list(self.mlp.activations))}
        for i, (w, b) in enumerate(zip(self.mlp.weights, self.mlp.biases)):
            arrays[f"W{i}"] = np.asarray(w, np.float32)
            arrays[f"b{i}"] = np.asarray(b, np.float32)
        np.savez(path, **arrays)
        return path


def load_model(path: str):
    if os.path.isdir(path):
        return DenseMLPModel(load_dense_mlp(path))
    if path.endswith(".joblib"):
        # a joblib file is a pickle: load only files you wrote or trust
        import joblib

        model = joblib.load(path)
        if is_sklearn_boost(model):
            return BoostModel(BoostTables.from_sklearn(model))
        if is_sklearn_svm(model):
            return SvmModel(SvmTables.from_sklearn(model))
        if not is_sklearn_trees(model):
            raise ValueError(f"{path} holds a {type(model).__name__}; expected a fitted "
                             "scikit-learn forest, tree, gradient-boosting, SVC or "
                             "LogisticRegression classifier")
        return ForestModel(ForestTables.from_sklearn(model))
    if path.endswith(".npz") or os.path.exists(path + ".npz"):
        d = np.load(path if path.endswith(".npz") else path + ".npz", allow_pickle=False)
        if "forest_tables" in d.files:
            return ForestModel(ForestTables.load(path if path.endswith(".npz") else path + ".npz"))
        if "boost_tables" in d.files:
            return BoostModel(BoostTables.load(path if path.endswith(".npz") else path + ".npz"))
        if "svm_tables" in d.files:
            return SvmModel(SvmTables.load(path if path.endswith(".npz") else path + ".npz"))
        n = sum(1 for k in d.files if k.startswith("W"))
        return DenseMLPModel(DenseMLP([d[f"W{i}"] for i in range(n)],
                                      [d[f"b{i}"] for i in range(n)],
                                      [str(a) for a in d["activations"]]))
    alt = path.replace(".model", ".npz")
    if alt != path and os.path.exists(alt):
        return load_model(alt)
    raise FileNotFoundError(path)


class Classifier:
    """Wrapper for classifier having a predict_proba method (classifier.py:11-41)."""

    def __init__(self, classifier, n_jobs=1, verbose=0) -> None:
        if hasattr(classifier, "predict_proba") and callable(getattr(classifier, "predict_proba")):
            self._classifier = classifier
        else:
            raise ValueError("The provided model does not have methods 'predict_proba'.")

    def predict_proba(self, x: np.ndarray) -> np.ndarray:
        proba = self._classifier.predict_proba(x)
        if proba.shape[1] == 1:
            proba = np.concatenate((1 - proba, proba), axis=1)
        return proba

    def dense_weights(self) -> DenseMLP:
        """Weights for the device GEMM chain (engine extension)."""
        if not hasattr(self._classifier, "dense_weights"):
            raise NotImplementedError(
                "the MI355X engine runs Dense-MLP classifiers (load_model); got "
                f"{type(self._classifier).__name__}")
        return self._classifier.dense_weights()

    def forest_tables(self) -> ForestTables:
        """Tables for the device tree walk (engine extension): the model is a fitted
        scikit-learn forest / tree classifier, a ForestTables or a ForestModel."""
        clf = self._classifier
        if callable(getattr(clf, "forest_tables", None)):
            return clf.forest_tables()
        if is_sklearn_trees(clf):
            if getattr(self, "_forest", None) is None:
                self._forest = ForestTables.from_sklearn(clf)
            return self._forest
        raise NotImplementedError(
            f"{type(clf).__name__} is not a tree ensemble the MI355X engine runs")

    def boost_tables(self) -> BoostTables:
        """Tables for the device walk of a boosted ensemble (engine extension): the model is a
        fitted scikit-learn GradientBoostingClassifier / HistGradientBoostingClassifier, a
        BoostTables or a BoostModel."""
        clf = self._classifier
        if callable(getattr(clf, "boost_tables", None)):
            return clf.boost_tables()
        if is_sklearn_boost(clf):
            if getattr(self, "_boost", None) is None:
                self._boost = BoostTables.from_sklearn(clf)
            return self._boost
        raise NotImplementedError(
            f"{type(clf).__name__} is not a boosted ensemble the MI355X engine runs")

    def svm_tables(self) -> SvmTables:
        """Tables for the device run of a kernel machine or logistic regression (engine
        extension): the model is a fitted scikit-learn SVC / NuSVC / LogisticRegression within
        the engine's limits, an SvmTables or an SvmModel."""
        clf = self._classifier
        if callable(getattr(clf, "svm_tables", None)):
            return clf.svm_tables()
        if is_sklearn_svm(clf):
            if getattr(self, "_svm", None) is None:
                self._svm = SvmTables.from_sklearn(clf)
            return self._svm
        raise NotImplementedError(
            f"{type(clf).__name__} is not a kernel machine or logistic regression the MI355X "
            "engine runs")
