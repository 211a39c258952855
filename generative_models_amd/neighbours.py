"""Nearest training neighbours of images, in pixel space (an extension; the reference has no counterpart): are the samples new images or
copies of training images?  No kernel code here - the search is ops.nn_search_u8, exact integer arithmetic on the bytes (include/gmk.h:
gmk_nn_search_u8), so every index and distance below is a function of the inputs alone.  tests/nn_ref.py restates all of it in numpy."""
import numpy as np
import torch

from . import ops


class NeighbourIndex:
    """A set of images held on the device as bytes (uint8 [N, ...], e.g. DeviceDataset.images), with the norms the search wants of its
    database computed once."""

    def __init__(self, images_u8):
        if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() < 2 or not images_u8.is_cuda:
            raise ValueError(f"NeighbourIndex: {getattr(images_u8, 'dtype', type(images_u8))} {tuple(getattr(images_u8, 'shape', ()))}, expected "
                             f"a uint8 device tensor [N, ...]")
        self.image_shape = tuple(images_u8.shape[1:])
        self.rows = images_u8.reshape(images_u8.shape[0], -1).contiguous()          # [N, D]
        self.sqnorm = ops.u8_sqnorm(self.rows)

    def __len__(self):
        return self.rows.shape[0]

    @property
    def D(self):
        return self.rows.shape[1]

    def search(self, queries_u8, k=1, mirror=False):
        """-> (dist2 int32 [Q, k], index int64 [Q, k], mirrored bool [Q]).  queries_u8: uint8 [Q, *image_shape] on the device.  mirror: every
        query is also searched flipped along W (its last dimension) - d(q, flip(x)) = d(flip(q), x), so this finds mirrored training images
        without a second database.  Per query the orientation with the smaller first pair (d2, j) wins, the unmirrored one on a tie, and its
        whole k-list is returned; `mirrored` says which."""
        if tuple(queries_u8.shape[1:]) != self.image_shape:
            raise ValueError(f"NeighbourIndex.search: queries of shape {tuple(queries_u8.shape)}, the index holds images of {self.image_shape}")
        dist2, index = ops.nn_search_u8(queries_u8, self.rows, k, self.sqnorm)
        mirrored = torch.zeros((queries_u8.shape[0],), dtype=torch.bool, device=dist2.device)
        if mirror:
            dist2_m, index_m = ops.nn_search_u8(queries_u8.flip(-1), self.rows, k, self.sqnorm)
            mirrored = (dist2_m[:, 0] < dist2[:, 0]) | ((dist2_m[:, 0] == dist2[:, 0]) & (index_m[:, 0] < index[:, 0]))
            dist2 = torch.where(mirrored[:, None], dist2_m, dist2)
            index = torch.where(mirrored[:, None], index_m, index)
        return dist2, index, mirrored


def rms_distance(dist2_first, D):
    """mean over the rows of sqrt(d2 / D) / 255, float64 on the host: the RMS difference per value as a fraction of the full range."""
    return float(np.mean(np.sqrt(np.asarray(dist2_first, dtype=np.float64) / D) / 255.0))


def lower_median(values):
    """sorted(values)[(n - 1) // 2]: an element of the list, so comparisons against it are exact."""
    v = np.sort(np.asarray(values).reshape(-1))
    return v[(v.size - 1) // 2]


def nn_report(index, samples_u8, holdout_u8, k=1, mirror=False):
    """How close `samples_u8` lie to the indexed (training) set, calibrated by how close held-out real images lie to it -> dict:
      nn_dist       rms_distance of the samples' nearest-neighbour distances
      nn_dist_test  the same of the held-out images'
      nn_closer     the fraction of samples whose nearest distance d2 is strictly below the lower median of the held-out images' - about 0.5
                    for a model that generalises, towards 1 for one that copies its training set
      index int64 [Q, k], dist2 int32 [Q, k], mirrored bool [Q]: the samples' neighbours; test_dist2 int32 [Q_test]: the held-out images' d2
    (arrays on the host)."""
    dist2, idx, mirrored = index.search(samples_u8, k, mirror)
    dist2_t, _, _ = index.search(holdout_u8, 1, mirror)
    dist2, idx, mirrored, dist2_t = dist2.cpu().numpy(), idx.cpu().numpy(), mirrored.cpu().numpy(), dist2_t[:, 0].cpu().numpy()
    return {"nn_dist": rms_distance(dist2[:, 0], index.D), "nn_dist_test": rms_distance(dist2_t, index.D),
            "nn_closer": float(np.mean(dist2[:, 0] < lower_median(dist2_t))),
            "index": idx, "dist2": dist2, "mirrored": mirrored, "test_dist2": dist2_t}
