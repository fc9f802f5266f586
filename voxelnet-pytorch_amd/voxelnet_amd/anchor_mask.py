"""SECOND's anchor mask (`anchor_area_threshold`; csrc/anchor_mask.hip): an anchor over whose bird's-eye
footprint the frame has (almost) no occupied voxel is ignored by the loss (pos = neg = 0) and can never become a detection
(its score is 0 in a copy of the probability map).  Host side, once per anchor set: every anchor's inclusive cell
rectangle on the voxel grid (`anchor_cell_rects`, NumPy float64).  Device side, every step: the voxels per BEV cell, their
summed-area table and four reads per anchor (`vn_anchor_mask`) — integers throughout, exact and bit-identical from run to
run.  There is no CPU path.

`RPN3D(anchor_area_threshold=1)` applies it to the targets the model generates itself and to what `evaluate` / `predict`
decode; caller-supplied `targets=` and a `target_fn` are not edited — `AnchorMasker` is public for those callers."""
import numpy as np
import torch

from . import _lib
from .config import grid_config
from .targets import generate_anchors

SNAP = 1e-9          # a rectangle edge within SNAP cells of a cell boundary IS that boundary
LAYOUTS = {"flat": _lib.VN_DETECT_FLAT, "site": _lib.VN_DETECT_SITE}


def check_threshold(threshold):
    """ValueError unless threshold is an integer >= 0 (what the library answers with VN_EINVAL), raised on the host"""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, np.integer)) or not 0 <= threshold < 2 ** 31:
        raise ValueError(f"anchor_area_threshold must be an integer >= 0, not {threshold!r}")
    return int(threshold)


def anchor_cell_rects(anchors, grid):
    """anchors (..., 7) float64 [x, y, z, h, w, l, r], grid a config.GridConfig -> (N, 4) int32 [w0, h0, w1, h1], the inclusive
    cell rectangle of every anchor's axis-aligned footprint on the (H, W) grid, in the anchors' flat order (n = 2 * site + a):
      ex = (|cos r| l + |sin r| w) / 2,  ey = (|sin r| l + |cos r| w) / 2
      q  = [(x - ex + ox) / vx, (y - ey + oy) / vy, (x + ex + ox) / vx, (y + ey + oy) / vy]       in cells
      a component within 1e-9 of an integer is that integer (an edge ON a cell boundary, up to float64 noise)
      half-open footprint: w0 = floor(q0), h0 = floor(q1), w1 = ceil(q2) - 1, h1 = ceil(q3) - 1, clipped to the grid.
    An anchor whose unclipped rectangle misses the grid or is empty (or has a non-finite field) is stored as [0, 0, -1, -1]:
    w1 < w0, count 0."""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    x, y, w, l, r = a[:, 0], a[:, 1], a[:, 4], a[:, 5], a[:, 6]
    ox, oy, vx, vy = float(grid.ox), float(grid.oy), float(grid.vx), float(grid.vy)
    with np.errstate(invalid="ignore", over="ignore"):          # (a non-finite field: the anchor is stored empty below)
        c, s = np.abs(np.cos(r)), np.abs(np.sin(r))
        ex, ey = (c * l + s * w) / 2, (s * l + c * w) / 2
        q = np.stack([(x - ex + ox) / vx, (y - ey + oy) / vy, (x + ex + ox) / vx, (y + ey + oy) / vy], axis=1)
    ok = np.isfinite(q).all(axis=1)
    q = np.where(ok[:, None], q, 0.0)
    near = np.rint(q)
    q = np.where(np.abs(q - near) <= SNAP, near, q)
    lo, hi = np.floor(q[:, :2]), np.ceil(q[:, 2:]) - 1
    top = np.array([grid.W - 1, grid.H - 1], dtype=np.float64)
    ok &= (hi >= lo).all(axis=1) & (hi >= 0).all(axis=1) & (lo <= top).all(axis=1)
    rect = np.concatenate([np.clip(lo, 0, top), np.clip(hi, 0, top)], axis=1)
    rect[~ok] = (0, 0, -1, -1)
    return np.ascontiguousarray(rect.astype(np.int32))


class AnchorMasker:
    """Device-resident cell rectangles of one anchor set + the launches.  anchors: (h, w, 2, 7) float64 (default: the class's,
    targets.generate_anchors); threshold: an anchor is kept when MORE than `threshold` voxels lie over its footprint (SECOND's
    value: 1; 0 keeps every anchor with a voxel under it); grid: the voxel grid the coordinates index (default: the
    class's, config.grid_config).  The anchor grid (h, w) and the BEV grid (H, W) are related through the metric coordinates
    only."""

    def __init__(self, cls_name="Car", device="cuda:0", anchors=None, threshold=1, grid=None):
        self.threshold = check_threshold(threshold)
        self.cls_name = cls_name
        self.grid = grid_config(cls_name) if grid is None else grid
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.VoxelnetHipError("AnchorMasker needs a HIP device (no CPU path)")
        self.anchors = generate_anchors(cls_name) if anchors is None else np.asarray(anchors, dtype=np.float64)
        if self.anchors.ndim != 4 or self.anchors.shape[2:] != (2, 7):
            raise ValueError(f"anchors {self.anchors.shape} are not (h, w, 2, 7)")
        self.shape = self.anchors.shape[:2]
        self.rects = anchor_cell_rects(self.anchors, self.grid)
        self._rects_dev = torch.from_numpy(self.rects).to(self.device)
        self.n_anchors = self.rects.shape[0]

    def mask(self, coord, B, return_count=False, pos=None, neg=None):
        """coord: the batch's concatenated (K, 4) int64 voxel coordinates [b, d, h, w] on the device (K may be 0); B samples
        -> mask (B, h, w, 2) uint8, 1 = kept [, count (B, h, w, 2) int32: the voxels over every anchor's footprint].  pos / neg:
        a (B, h, w, 2) float32 pair edited IN PLACE — zero where the anchor is masked out, not written where it is kept.
        Enqueued on the current stream, no host synchronisation."""
        if not (torch.is_tensor(coord) and coord.is_cuda):
            raise _lib.VoxelnetHipError("AnchorMasker.mask: coord must be a tensor on a HIP device (no CPU path)")
        if coord.dim() != 2 or coord.shape[1] != 4 or coord.dtype != torch.int64:
            raise ValueError(f"AnchorMasker.mask: coord {tuple(coord.shape)} {coord.dtype} is not (K, 4) int64")
        if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or B < 1:
            raise ValueError(f"AnchorMasker.mask: B must be a positive integer, not {B!r}")
        B, N, dev = int(B), self.n_anchors, coord.device
        if (pos is None) != (neg is None):
            raise ValueError("AnchorMasker.mask: pos and neg come as a pair")
        for name, t in (("pos", pos), ("neg", neg)):
            if t is None:
                continue
            if not (torch.is_tensor(t) and t.is_cuda):
                raise _lib.VoxelnetHipError(f"AnchorMasker.mask: {name} must be a tensor on a HIP device (no CPU path)")
            if tuple(t.shape) != (B, *self.shape, 2) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"AnchorMasker.mask: {name} {tuple(t.shape)} {t.dtype} is not a contiguous "
                                 f"{(B, *self.shape, 2)} float32 tensor on {dev}")
        coord = coord.contiguous()
        g = self.grid
        nbytes = _lib.load().vn_anchor_mask_workspace_bytes(B, g.H, g.W, N)
        if nbytes == 0:
            raise _lib.VoxelnetHipError("vn_anchor_mask_workspace_bytes: unsupported sizes")
        mask = torch.empty((B, *self.shape, 2), dtype=torch.uint8, device=dev)
        count = torch.empty((B, *self.shape, 2), dtype=torch.int32, device=dev) if return_count else None
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            _lib.call("vn_anchor_mask", coord.data_ptr() if coord.shape[0] else None, coord.shape[0], B, g.H, g.W,
                      self._rects_dev.data_ptr(), N, self.threshold, mask.data_ptr(), count.data_ptr() if return_count else None,
                      None if pos is None else pos.data_ptr(), None if neg is None else neg.data_ptr(), ws.data_ptr(), nbytes,
                      _lib.raw_stream())
        return (mask, count) if return_count else mask

    def mask_probs(self, probs, mask, layout="flat"):
        """probs (B, 2, h, w) float32 and a (B, h, w, 2) uint8 mask -> a COPY of probs in which every masked-out anchor's score
        is 0, in the layout the decode reads ("flat": anchor n <-> probs[b].flat[n]; "site": anchor n = 2 s + a <->
        probs[b, a, s]); kept elements are bit-identical, the input is untouched."""
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, not {layout!r}")
        return mask_probs(probs, mask, self.n_anchors, LAYOUTS[layout])


def mask_probs(probs, mask, n_anchors, layout):
    """vn_anchor_mask_probs on probs (B, ...) with n_anchors elements per sample and mask (B, ...) uint8 with as many;
    layout: VN_DETECT_FLAT / VN_DETECT_SITE"""
    for name, t in (("probs", probs), ("anchor_mask", mask)):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.VoxelnetHipError(f"mask_probs: {name} must be a tensor on a HIP device (no CPU path)")
    B = probs.shape[0] if probs.dim() else 0
    if B < 1 or probs.numel() != B * n_anchors or probs.dtype != torch.float32:
        raise ValueError(f"mask_probs: probs {tuple(probs.shape)} {probs.dtype} is not float32 with {n_anchors} anchors per sample")
    if mask.dim() < 1 or mask.shape[0] != B or mask.numel() != B * n_anchors or mask.dtype != torch.uint8 or mask.device != probs.device:
        raise ValueError(f"mask_probs: anchor_mask {tuple(mask.shape)} {mask.dtype} is not a uint8 mask of {B} x {n_anchors} "
                         f"anchors on {probs.device}")
    probs, mask = probs.detach().contiguous(), mask.contiguous()
    out = torch.empty_like(probs)
    with _lib.on_device(probs.device):
        _lib.call("vn_anchor_mask_probs", probs.data_ptr(), mask.data_ptr(), B, n_anchors, layout, out.data_ptr(), _lib.raw_stream())
    return out
