"""Writes tests/golden/knn_impute.npz: the inputs of knn_impute_ref.cpu_cases() and what the installed
sklearn.impute.KNNImputer(n_neighbors=k) makes of them in float64 (fit on ``fit``, transform of ``q``; the case ``self``
is fit_transform).  Run from the repository root:  python tests/golden/make_knn_impute_golden.py"""
import os
import sys

import numpy as np
import sklearn
from sklearn.impute import KNNImputer

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from knn_impute_ref import cpu_cases  # noqa: E402


def main():
    store = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (fit, q, k) in cpu_cases().items():
        imp = KNNImputer(n_neighbors=k)
        out = imp.fit_transform(fit) if name == "self" else imp.fit(fit).transform(q)
        store[name + "/fit"], store[name + "/q"], store[name + "/k"], store[name + "/out"] = fit, q, np.array(k), out
    np.savez_compressed(os.path.join(HERE, "knn_impute.npz"), **store)


if __name__ == "__main__":
    main()
