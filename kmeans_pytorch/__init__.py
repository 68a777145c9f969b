"""Drop-in stand-in for ``kmeans_pytorch.kmeans`` (the unpinned pip package the reference imports in gui.py and
gui_standalone.py), backed by the HIP Lloyd loop of trase_amd.segment.

Same signature and return as the library's 0.3 release: ``(ids.cpu(), centres.cpu())``.  Only what the reference uses is
provided: euclidean distance, random start rows (``cluster_centers=[]``), a CUDA ``device``.  An empty cluster is re-seeded
by a hash of (seed or one torch CPU draw, iteration, cluster) instead of the library's ``torch.randint`` (see
trase_amd/segment.py)."""
import torch

from trase_amd.segment import kmeans as _kmeans

__all__ = ["kmeans"]


def kmeans(X, num_clusters, distance='euclidean', cluster_centers=[], tol=1e-4, tqdm_flag=True, iter_limit=0,
           device=torch.device('cpu'), gamma_for_soft_dtw=0.001, seed=None):
    if distance != 'euclidean':
        raise NotImplementedError(f"kmeans_pytorch shim: distance={distance!r} (only 'euclidean' is provided)")
    if not (isinstance(cluster_centers, list) and len(cluster_centers) == 0):
        raise NotImplementedError("kmeans_pytorch shim: explicit cluster_centers are not provided")
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(f"kmeans_pytorch shim: runs on the GPU only (device={device}; there is no CPU path)")
    if tqdm_flag:
        print(f'running k-means on {device}..')
    ids, centres, _ = _kmeans(X.float().to(device), num_clusters, tol=tol, iter_limit=iter_limit, seed=seed)
    return ids.cpu(), centres.cpu()
