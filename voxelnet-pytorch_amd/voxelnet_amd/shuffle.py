"""The per-sample point shuffle of the input pipeline — the reference's `np.random.shuffle(point_cloud)` in front of the
voxelizer (voxelnet/utils.py:35), which decides which <= T points of a crowded voxel survive — split where the work splits:

  host   (this module): the DRAW.  `draw_index(n)` shuffles arange(n) with the global np.random: the same Mersenne-Twister
         draws as the shuffle of the (n,C) cloud itself, so cloud[index] is the reference's shuffled cloud bit for bit and
         np.random is left where the reference leaves it — at a fraction of the cost (NumPy shuffles a 2-D array row by row
         through its generic swap path).  `draw_keys()` draws six uint32 for the keyed form: no host work proportional to n.
  device (csrc/shuffle.hip): the GATHER of the rows, on the pipeline's stream right behind the host->device copy —
         `vn_permute_points` (out[i] = points[index[i]]) and `vn_shuffle_points` (out[i] = points[p(i)], p a six-round
         Feistel bijection of [0, n) under the keys, walked until it lands inside the range; include/voxelnet_hip.h states
         it).  There is no CPU path for the points.

`DeviceCollate(..., shuffle_points="index" | "device")` / `DeviceBatcher` (dataset.py) run one pair per sample."""
import numpy as np
import torch

from . import _lib


def draw_index(n):
    """(n,) int32: arange(n) shuffled by the global np.random.shuffle — cloud[draw_index(len(cloud))] equals
    np.random.shuffle(cloud) from the same state, and the state afterwards is the same"""
    index = np.arange(int(n), dtype=np.int32)
    np.random.shuffle(index)
    return index


def draw_keys():
    """(6,) uint32 round keys of vn_shuffle_points: ONE call of the global np.random.randint"""
    return np.random.randint(0, 2 ** 32, 6, dtype=np.uint32)


def _check(points, out, what):
    if not (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2
            and points.shape[1] == 4 and points.is_contiguous()):
        raise _lib.VoxelnetHipError(f"{what} needs a contiguous (N,4) float32 HIP tensor (there is no CPU path)")
    if out is None:
        return torch.empty_like(points)
    if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == points.shape
            and out.is_contiguous() and out.device == points.device):
        raise _lib.VoxelnetHipError(f"{what}: out must be a contiguous float32 HIP tensor of the points' shape")
    return out


def enqueue_permute_points(points, index, out=None):
    """out[i] = points[index[i]] on the current stream.  index: n integers on the host (staged through pinned memory and
    copied asynchronously, as augment.enqueue_augment_points stages its table) or an int32 HIP tensor already on the points'
    device.  An index outside [0, n) gives a NaN point.  `out` must not be `points`.
    -> (out, tensors the queued work reads: keep them referenced until the stream has run it)"""
    out = _check(points, out, "permute_points_device")
    dev = points.device
    n = points.shape[0]
    keep = (points,)
    with _lib.on_device(dev):
        if torch.is_tensor(index):
            if not (index.is_cuda and index.device == dev and index.dtype == torch.int32 and index.dim() == 1
                    and index.shape[0] == n and index.is_contiguous()):
                raise _lib.VoxelnetHipError("permute_points_device: a device index must be a contiguous (N,) int32 tensor on the points' device")
            table = index
        else:
            index = np.ascontiguousarray(index, dtype=np.int32)
            if index.shape != (n,):
                raise ValueError(f"index has shape {index.shape}; the cloud has {n} rows")
            # pinned staging + an asynchronous copy on the current stream: a copy from pageable memory would make the
            # host wait for everything queued in front of it
            host = torch.from_numpy(index).pin_memory() if n else torch.from_numpy(index)
            table = host.to(dev, non_blocking=True)
            keep += (host,)
        keep += (table,)
        _lib.call("vn_permute_points", points.data_ptr(), n, table.data_ptr(), out.data_ptr(), _lib.raw_stream())
    return out, keep


def enqueue_shuffle_points(points, keys, out=None):
    """out[i] = points[p(i)] on the current stream, p the bijection of [0, n) under the six uint32 `keys` (draw_keys()).
    The keys travel as a kernel argument — the library reads them during the call — so there is no table to stage and
    no copy.  `out` must not be `points`.  -> (out, what the queued work reads, as enqueue_permute_points)"""
    out = _check(points, out, "shuffle_points_device")
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    if keys.shape != (6,):
        raise ValueError(f"keys has shape {keys.shape}; vn_shuffle_points takes six uint32")
    with _lib.on_device(points.device):
        _lib.call("vn_shuffle_points", points.data_ptr(), points.shape[0], keys.ctypes.data, out.data_ptr(), _lib.raw_stream())
    return out, (points, keys)


def permute_points_device(points, index, out=None):
    """points: contiguous (N,4) float32 HIP tensor -> the rows in the order of `index` (`out`; a new tensor when None),
    bit copies, enqueued on the current stream without any host synchronisation.  Raises VoxelnetHipError for anything
    but a HIP tensor: the per-point work has no CPU path."""
    return enqueue_permute_points(points, index, out)[0]


def shuffle_points_device(points, keys, out=None):
    """points: contiguous (N,4) float32 HIP tensor -> the rows in the order of the keyed bijection, as
    permute_points_device"""
    return enqueue_shuffle_points(points, keys, out)[0]
