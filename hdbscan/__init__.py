"""Drop-in stand-in for the ``hdbscan`` package as the reference uses it (gui.py:280-282, gui_standalone.py:721-727):
``hdbscan.HDBSCAN(min_cluster_size=10, cluster_selection_epsilon=0.01, allow_single_cluster=False,
core_dist_n_jobs=...).fit_predict(ndarray)``, backed by the HIP kernels of trase_amd.segment.hdbscan.

Only what that call needs is provided: the euclidean metric, excess-of-mass selection, ``fit`` / ``fit_predict`` and
``labels_``.  The array is uploaded to the current CUDA device; there is no CPU path.  Among exactly equal distances the
spanning tree follows our edge order, not the package's, and the clusters are numbered by their smallest member index
(see trase_amd/segment.py)."""
import numpy as np
import torch

from trase_amd.segment import hdbscan as _hdbscan

__all__ = ["HDBSCAN"]


class HDBSCAN:
    def __init__(self, min_cluster_size=5, min_samples=None, cluster_selection_epsilon=0.0, allow_single_cluster=False,
                 metric='euclidean', cluster_selection_method='eom', alpha=1.0, core_dist_n_jobs=4, **ignored):
        if metric != 'euclidean':
            raise NotImplementedError(f"hdbscan shim: metric={metric!r} (only 'euclidean' is provided)")
        if cluster_selection_method != 'eom':
            raise NotImplementedError(f"hdbscan shim: cluster_selection_method={cluster_selection_method!r} "
                                      "(only 'eom' is provided)")
        if float(alpha) != 1.0:
            raise NotImplementedError(f"hdbscan shim: alpha={alpha!r} (only 1.0 is provided)")
        self.min_cluster_size = min_cluster_size
        self.min_samples = min_samples
        self.cluster_selection_epsilon = cluster_selection_epsilon
        self.allow_single_cluster = allow_single_cluster
        self.metric = metric
        self.cluster_selection_method = cluster_selection_method
        self.core_dist_n_jobs = core_dist_n_jobs        # accepted and unused: the distances are computed on the GPU
        self.labels_ = None

    def fit(self, X, y=None):
        if not torch.cuda.is_available():
            raise RuntimeError("hdbscan shim: runs on the GPU only (there is no CPU path)")
        X = np.ascontiguousarray(np.asarray(X), dtype=np.float32)
        if X.ndim != 2:
            raise ValueError(f"hdbscan shim: X must be (n, D), got {X.shape}")
        labels = _hdbscan(torch.from_numpy(X).cuda(), min_cluster_size=self.min_cluster_size, min_samples=self.min_samples,
                          cluster_selection_epsilon=self.cluster_selection_epsilon,
                          allow_single_cluster=self.allow_single_cluster)
        self.labels_ = labels.cpu().numpy()
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_
