"""Test-time augmentation and box voting for the detection tail (csrc/tta.hip).

The greedy NMS of section 1c keeps the best-scoring box of a cluster and drops its near-duplicates.  Two refinements every
SECOND-family evaluation applies after it:

* box voting — `vote_device` (`vn_box_vote`): every kept row becomes the score- (and IoU-) weighted mean of the rows of the
  pool that overlap it by at least `BoxVote.thres`; `BoxDecoder.decode_device(..., vote=BoxVote())` composes it into the tail.
* test-time augmentation — `TestTimeAugment`: the frame is run once per `View` (flipped, rotated, scaled by
  `vn_augment_compose`), each view's candidates are decoded on their own, `merge_pools` (`vn_pool_merge`) maps them back to
  the frame's coordinates and merges them into one priority order, and the NMS and the vote run on the merged pool:
  `RPN3D.evaluate(..., tta=TestTimeAugment())`, `RPN3D.predict(..., tta=...)`.

Everything runs on the device and nothing here waits for it; there is no CPU path."""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

WEIGHTS = {"score": _lib.VN_VOTE_W_SCORE, "score_iou": _lib.VN_VOTE_W_SCORE_IOU}
SCORES = {"keep": _lib.VN_VOTE_S_KEEP, "view_mean": _lib.VN_VOTE_S_VIEW_MEAN}


@dataclass(frozen=True)
class View:
    """one view of a frame: y -> -y when flip_y, then a rotation by -angle about the lidar origin, then a scaling — stages
    2-4 of augment.compose_affine, no translation.  View() is the identity."""
    flip_y: bool = False
    angle: float = 0.0
    scale: float = 1.0

    def __post_init__(self):
        if not isinstance(self.flip_y, (bool, np.bool_)):
            raise ValueError(f"View.flip_y must be a bool, not {self.flip_y!r}")
        if not (isinstance(self.angle, (int, float, np.floating, np.integer)) and math.isfinite(self.angle)):
            raise ValueError(f"View.angle must be finite, not {self.angle!r}")
        if not (isinstance(self.scale, (int, float, np.floating, np.integer)) and math.isfinite(self.scale)
                and float(np.float32(self.scale)) > 0 and math.isfinite(float(np.float32(self.scale)))):
            raise ValueError(f"View.scale must be finite and > 0, not {self.scale!r}")

    @property
    def identity(self):
        return not self.flip_y and float(self.angle) == 0.0 and float(np.float32(self.scale)) == 1.0

    def row(self):
        """(fy, angle, factor) as vn_pool_merge takes it; the factor is the float32 the points were scaled by
        (augment.compose_affine rounds it the same way)"""
        return (-1.0 if self.flip_y else 1.0, float(self.angle), float(np.float32(self.scale)))


@dataclass(frozen=True)
class BoxVote:
    """thres: the BEV IoU with the kept row from which a row of the pool is a member of its cluster (> 0);
    weight: "score_iou" (w = s * IoU, CIA-SSD's weighted NMS) or "score" (w = s);
    score: "keep" (the kept row's score) or "view_mean" (the mean over the views of each view's best member score, 0 for
    a view that did not see the object)."""
    thres: float = 0.5
    weight: str = "score_iou"
    score: str = "keep"

    def __post_init__(self):
        if not (isinstance(self.thres, (int, float, np.floating, np.integer)) and math.isfinite(self.thres) and self.thres > 0):
            raise ValueError(f"BoxVote.thres must be finite and > 0, not {self.thres!r}")
        if self.weight not in WEIGHTS:
            raise ValueError(f"BoxVote.weight must be one of {sorted(WEIGHTS)}, not {self.weight!r}")
        if self.score not in SCORES:
            raise ValueError(f"BoxVote.score must be one of {sorted(SCORES)}, not {self.score!r}")


def _view_rows(views):
    """views: View objects or (fy, angle, factor) rows -> (V,3) float64, checked as vn_pool_merge checks it"""
    rows = [v.row() if isinstance(v, View) else tuple(float(x) for x in v) for v in views]
    arr = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, 3))
    if not 1 <= arr.shape[0] <= _lib.VN_TTA_MAX_VIEWS:
        raise ValueError(f"{arr.shape[0]} views; want 1 .. {_lib.VN_TTA_MAX_VIEWS}")
    if not (np.isin(arr[:, 0], (1.0, -1.0)).all() and np.isfinite(arr[:, 1:]).all() and (arr[:, 2] > 0).all()):
        raise ValueError("a view is (fy = +1 or -1, a finite angle, a finite factor > 0)")
    return arr


def _stacked(x, what):
    if isinstance(x, (list, tuple)):
        if not all(torch.is_tensor(t) and t.is_cuda for t in x):
            raise _lib.VoxelnetHipError(f"merge_pools: {what} must be HIP tensors (no CPU path)")
        x = torch.stack(list(x))
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.VoxelnetHipError(f"merge_pools: {what} must be HIP tensors (no CPU path)")
    return x


def merge_pools(boxes, scores, counts, views):
    """The candidate pools of V views of one batch as ONE pool in the frame's own coordinates (vn_pool_merge): boxes (V,B,K,7)
    f32, scores (V,B,K) f32, counts (V,B) int32 — stacked device tensors or lists of V per-view tensors, what
    BoxDecoder.candidates_device returns per view — and `views`, V View objects (or (fy, angle, factor) rows) ->
    (boxes (B,V*K,7) f32, scores (B,V*K) f32, src (B,V*K) int32 = view * K + row, counts (B,) int32) on the device: per sample
    the rows in descending score, equal scores with the smaller src first, a NaN score dropped; rows past the count are zero.
    Enqueued on the current stream, no host synchronisation."""
    boxes, scores, counts = _stacked(boxes, "boxes"), _stacked(scores, "scores"), _stacked(counts, "counts")
    vr = _view_rows(views)
    if boxes.dim() != 4 or boxes.shape[3] != 7 or scores.shape != boxes.shape[:3] or counts.shape != boxes.shape[:2]:
        raise ValueError(f"boxes {tuple(boxes.shape)} / scores {tuple(scores.shape)} / counts {tuple(counts.shape)}: want "
                         "(V,B,K,7), (V,B,K) and (V,B)")
    V, B, K = boxes.shape[:3]
    if V != vr.shape[0]:
        raise ValueError(f"{V} pools for {vr.shape[0]} views")
    if B < 1 or K < 1 or V * K > _lib.VN_DETECT_MAX_PRE:
        raise ValueError(f"V = {V}, B = {B}, K = {K}: want B >= 1, K >= 1 and V * K <= {_lib.VN_DETECT_MAX_PRE}")
    boxes, scores = boxes.detach().float().contiguous(), scores.detach().float().contiguous()
    counts = counts.to(torch.int32).contiguous()
    dev = boxes.device
    ob = torch.zeros((B, V * K, 7), dtype=torch.float32, device=dev)
    os_ = torch.zeros((B, V * K), dtype=torch.float32, device=dev)
    src = torch.zeros((B, V * K), dtype=torch.int32, device=dev)
    oc = torch.zeros(B, dtype=torch.int32, device=dev)
    nbytes = _lib.load().vn_pool_merge_workspace_bytes(V, B, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.call("vn_pool_merge", boxes.data_ptr(), scores.data_ptr(), counts.data_ptr(), vr.ctypes.data, V, B, K, ob.data_ptr(),
                  os_.data_ptr(), src.data_ptr(), oc.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
    return ob, os_, src, oc


def vote_device(boxes, scores, counts, keep_idx, keep_counts, vote, src=None, rows_per_view=None, n_views=1):
    """Box voting behind predict.nms_device (vn_box_vote): boxes (B,K,7) f32 / scores (B,K) f32 / counts (B,) int32 — the pool
    the NMS walked — and its keep_idx (B,P) int32 / keep_counts (B,) int32, all device tensors; vote: a BoxVote.
    src (B,K) int32 with rows_per_view and n_views: merge_pools' src and its K and V — row j is view src[j] // rows_per_view
    (needed by score="view_mean" over more than one view); None: every row is view 0 and n_views must be 1.
    -> (boxes (B,P,7) f32, scores (B,P) f32, counts (B,) int32, members (B,P) int32) on the device: the voted rows in descending
    output score, rows past the count zero.  Enqueued on the current stream, no host synchronisation."""
    if not isinstance(vote, BoxVote):
        raise ValueError(f"vote must be a tta.BoxVote, not {vote!r}")
    ts = [boxes, scores, counts, keep_idx, keep_counts] + ([] if src is None else [src])
    if not all(torch.is_tensor(t) and t.is_cuda for t in ts):
        raise _lib.VoxelnetHipError("vote_device: every tensor must be a HIP tensor (no CPU path)")
    if boxes.dim() != 3 or boxes.shape[2] != 7 or scores.shape != boxes.shape[:2] or counts.shape != boxes.shape[:1]:
        raise ValueError(f"boxes {tuple(boxes.shape)} / scores {tuple(scores.shape)} / counts {tuple(counts.shape)}: want (B,K,7), "
                         "(B,K) and (B,)")
    B, K = boxes.shape[:2]
    if keep_idx.dim() != 2 or keep_idx.shape[0] != B or keep_counts.shape != (B,):
        raise ValueError(f"keep_idx {tuple(keep_idx.shape)} / keep_counts {tuple(keep_counts.shape)}: want (B,P) and (B,)")
    P = keep_idx.shape[1]
    if not (1 <= B <= 65535 and 1 <= K <= _lib.VN_DETECT_MAX_PRE and 1 <= P <= _lib.VN_PREDICT_MAX_TOPK):
        raise ValueError(f"B = {B}, K = {K}, P = {P}: want 1 <= B <= 65535, 1 <= K <= {_lib.VN_DETECT_MAX_PRE}, "
                         f"1 <= P <= {_lib.VN_PREDICT_MAX_TOPK}")
    if not (isinstance(n_views, (int, np.integer)) and 1 <= n_views <= _lib.VN_TTA_MAX_VIEWS):
        raise ValueError(f"n_views must be an integer in [1, {_lib.VN_TTA_MAX_VIEWS}], not {n_views!r}")
    if src is None:
        if n_views != 1:
            raise ValueError("vote_device: more than one view needs src and rows_per_view (merge_pools' src and K)")
        rpv = 0
    else:
        if src.shape != (B, K):
            raise ValueError(f"src {tuple(src.shape)}: want ({B},{K})")
        if not (isinstance(rows_per_view, (int, np.integer)) and rows_per_view >= 1):
            raise ValueError(f"rows_per_view must be an integer >= 1, not {rows_per_view!r}")
        rpv = int(rows_per_view)
        src = src.to(torch.int32).contiguous()
    boxes, scores = boxes.detach().float().contiguous(), scores.detach().float().contiguous()
    counts, keep_counts = counts.to(torch.int32).contiguous(), keep_counts.to(torch.int32).contiguous()
    keep_idx = keep_idx.to(torch.int32).contiguous()
    dev = boxes.device
    ob = torch.zeros((B, P, 7), dtype=torch.float32, device=dev)
    os_ = torch.zeros((B, P), dtype=torch.float32, device=dev)
    om = torch.zeros((B, P), dtype=torch.int32, device=dev)
    oc = torch.zeros(B, dtype=torch.int32, device=dev)
    nbytes = _lib.load().vn_box_vote_workspace_bytes(B, K, P, int(n_views))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.call("vn_box_vote", boxes.data_ptr(), scores.data_ptr(), counts.data_ptr(), None if src is None else src.data_ptr(), rpv,
                  keep_idx.data_ptr(), keep_counts.data_ptr(), B, K, P, int(n_views), float(vote.thres), WEIGHTS[vote.weight],
                  SCORES[vote.score], ob.data_ptr(), os_.data_ptr(), om.data_ptr(), oc.data_ptr(), ws.data_ptr(), nbytes,
                  _lib.raw_stream())
    return ob, os_, oc, om


@dataclass(frozen=True)
class TestTimeAugment:
    """views: the View objects a frame is run through (1 .. 8); vote: the BoxVote that fuses the merged pool (None: the
    merged pool goes through the NMS alone, which only picks a maximum); fov_calib_dir / image_shape: crop every view's raw
    cloud to the camera's field of view as dataset.DeviceCollate does (`<fov_calib_dir>/<tag>.txt`), for raw sweeps."""
    views: Tuple[View, ...] = (View(), View(flip_y=True))
    vote: Optional[BoxVote] = BoxVote(score="view_mean")
    fov_calib_dir: Optional[str] = None
    image_shape: Tuple[int, int] = (375, 1242)
    __test__ = False          # (not a test class, whatever its name says to pytest)

    def __post_init__(self):
        views = tuple(self.views)
        if not (1 <= len(views) <= _lib.VN_TTA_MAX_VIEWS and all(isinstance(v, View) for v in views)):
            raise ValueError(f"TestTimeAugment.views: 1 .. {_lib.VN_TTA_MAX_VIEWS} tta.View objects, not {self.views!r}")
        if self.vote is not None and not isinstance(self.vote, BoxVote):
            raise ValueError(f"TestTimeAugment.vote must be a tta.BoxVote or None, not {self.vote!r}")
        object.__setattr__(self, "views", views)
        object.__setattr__(self, "image_shape", tuple(self.image_shape))

    def view_points(self, view, cloud, tag, image, device):
        """one raw cloud (n, >= 4) numpy -> the (n,4) f32 device cloud of `view`, on the current stream: uploaded as is, cropped
        when fov_calib_dir is set, moved by vn_augment_compose with an empty move table"""
        from .augment import MOVE_DTYPE, ComposeParams, compose_affine, enqueue_compose_points
        host = torch.from_numpy(np.ascontiguousarray(np.asarray(cloud)[:, :4], dtype=np.float32)).pin_memory()
        pts = host.to(device, non_blocking=True)
        keep = (host,)
        if self.fov_calib_dir is not None:
            import os

            from .fov import fov_crop_device, load_calib
            P, Tr, R = load_calib(os.path.join(self.fov_calib_dir, str(tag) + ".txt"))
            rows, cols = image.shape[:2] if image is not None else self.image_shape
            pts, _ = fov_crop_device(pts, P, Tr, R, rows, cols, padded=True)
        _, angle, factor = view.row()
        none = np.zeros((0, 7))
        params = ComposeParams(none, none, np.zeros(0, dtype=bool), np.zeros(0, dtype=MOVE_DTYPE), [], bool(view.flip_y), angle, factor,
                               (0.0, 0.0, 0.0), compose_affine(bool(view.flip_y), angle, factor, None))
        pts, k2 = enqueue_compose_points(pts, params, out=pts)
        return pts, keep + tuple(k2)
