"""Input pipeline of the train loop with the voxelizer on the device — the reference's `KITTIDataset`
(voxelnet/dataset.py:26-67) and `collate_fn` / `prepare_voxel` (dataset.py:70-119) re-cut for the GPU:

  reference:  DataLoader worker: read .bin -> pcl_to_voxels on the CPU (0.2-0.8 s, utils.py:10-100) -> (K,T,7) buffers
              through the worker pipe -> collate -> `.to(device)` of 6-14 MB per sample (model.py:302-303)
  here:       DataLoader worker: read .bin / label / image only -> main process: shuffle (utils.py:35), ONE pinned
              host->device copy of the raw (N,4) cloud (0.3-2 MB) -> `vn_voxelize_index/gather` on a side stream,
              no host synchronisation -> the reference's 7-tuple with the voxel buffers already in HBM.

`DeviceBatcher` wraps any iterable of per-sample 5-tuples lists (a DataLoader with `collate_fn=list`) and keeps one
batch in flight: batch i+1 is copied and voxelized while batch i trains.

Data augmentation (dataset.py:122-219, `pcl_augmentation`: per-box perturbation, global rotation, global scaling) is a
stage of this pipeline, not of the dataset: copy -> [field-of-view crop] -> augment -> voxelize.  `DeviceCollate(...,
augment=True)` / `DeviceBatcher(..., augment=True)` draw the parameters per sample on the host (augment.py, after the
sample's shuffle), move the points on the device (csrc/augment.hip) and hand the model the moved label lines.  The
dataset itself runs in DataLoader workers, which must not touch the GPU: `KITTIDataset(augment=True)` still raises.
`augment=augment.ComposeRecipe(...)` selects the composed recipe instead (per-object noise, flip, global rotation, scaling,
translation for every sample; one launch, `vn_augment_compose`), drawn and launched at the same two places.

Ground-truth database sampling (gtsample.py; SECOND's "GT-paste", no counterpart in the reference) is the stage in front
of the augmentation: copy -> [field-of-view crop] -> paste -> augment -> voxelize.  `DeviceCollate(..., gt_sampler=s)` /
`DeviceBatcher(..., gt_sampler=s)` draw the pasted objects per sample on the host (after the sample's shuffle, before the
augmentation's draw, which then runs on the enlarged labels), paste their points on the device (csrc/gtsample.hip) and
hand the model labels + the pasted objects' lines.  A sampler with `visibility=gtsample.Visibility(...)` pastes with
`vn_gt_paste_visible` instead: objects hidden behind scene points are rejected on the device,
and `concat` drops their label lines once the sample's visible counts have arrived in pinned host memory.

Part-aware object augmentation (part_augment.py; SE-SSD / PA-AUG, no counterpart in the reference) is the stage between
the two: copy -> [field-of-view crop] -> paste -> parts -> augment -> voxelize.  `DeviceCollate(..., part_augment=
part_augment.PartRecipe())` draws per sample after the sampler and before the augmentation, on the labels including the
pasted lines, and drops, thins and swaps pyramids of the objects' points in place (csrc/part_augment.hip); the label lines
stay as they are.

The sample's shuffle (utils.py:35) is by default the reference's: `np.random.shuffle` of the host cloud, in the thread that
also enqueues the train step.  `shuffle_points="index"` / `"device"` move the per-point half to the device (shuffle.py,
csrc/shuffle.hip), as the first stage behind the copy: copy -> shuffle -> [field-of-view crop] -> paste -> augment ->
voxelize; the host then draws an index table (the same np.random draws, the same voxel buffers) or six round keys."""
import glob
import os

import numpy as np
import torch

from . import _lib
from .config import grid_config
from .voxelize import VoxelBatch, pipeline_stream, voxelize_device_async


def _read_image(path):
    """cv2.imread equivalent (dataset.py:50): HxWx3 uint8, BGR channel order; None when no decoder is installed"""
    try:
        from PIL import Image
    except ImportError:
        return None
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


class KITTIDataset(torch.utils.data.Dataset):
    """dataset.py:26-67 without the CPU voxelization: __getitem__ -> (tag, img, pcl (N,4) float32, labels, None)."""

    def __init__(self, data_dir, shuffle=True, augment=False, test=False, load_images=True):
        if augment:
            raise NotImplementedError("pcl_augmentation (dataset.py:122) runs on the device, not in dataset workers: use "
                                      "KITTIDataset(augment=False) with DeviceCollate / DeviceBatcher(..., augment=True)")
        self.data_dir, self.shuffle, self.test, self.load_images = data_dir, shuffle, test, load_images
        self.images = sorted(glob.glob(os.path.join(data_dir, "image_2") + "/*.png"))
        self.pcls = sorted(glob.glob(os.path.join(data_dir, "velodyne") + "/*.bin"))
        self.labels = sorted(glob.glob(os.path.join(data_dir, "label_2") + "/*.txt"))
        assert len(self.images) == len(self.pcls) == len(self.labels)          # dataset.py:40
        self.indices = list(range(len(self.images)))
        if self.shuffle:
            np.random.shuffle(self.indices)                                    # dataset.py:43-44

    def __len__(self):
        return len(self.images)

    def __getitem__(self, idx):
        index = self.indices[idx]
        tag = os.path.split(self.images[index])[1][:-4]                        # dataset.py:48
        img = _read_image(self.images[index]) if self.load_images else None
        pcl = np.fromfile(self.pcls[index], dtype=np.float32).reshape(-1, 4)   # dataset.py:51
        labels = [] if self.test else [line for line in open(self.labels[index], "r").readlines()]
        return tag, img, pcl, labels, None


def drop_rejected_lines(labels, n_pasted, visible, min_visible):
    """labels: a sample's label lines whose last `n_pasted` are pasted objects' (possibly moved by the augmentation: one
    line per input line, in order); visible: their visible counts (vn_gt_paste_visible's out_visible).  -> the lines
    without those of the rejected objects (visible < min_visible)"""
    visible = np.asarray(visible).reshape(-1)
    if visible.shape[0] != n_pasted or n_pasted > len(labels):
        raise ValueError(f"{visible.shape[0]} visible counts for {n_pasted} pasted lines of {len(labels)} label lines")
    first = len(labels) - n_pasted
    return list(labels[:first]) + [line for line, v in zip(labels[first:], visible) if v >= min_visible]


class DeviceCollate:
    """collate_fn (dataset.py:70-97) with pcl_to_voxels (utils.py:10-100) run on the device for the whole batch:
    parts = [(tag, img, pcl, labels, _)] -> the reference's 7-tuple, with x[2] / x[3] / x[4] = lists of DEVICE tensors
    feature (K_i,T,7) f32, number (K_i,) i64, coordinate (K_i,4) i64 [b,z,y,x].  Must run in the process that owns the
    GPU (not in a DataLoader worker)."""

    def __init__(self, device="cuda:0", target="Car", shuffle_points=True, fov_calib_dir=None, image_shape=(375, 1242),
                 augment=False, gt_sampler=None, part_augment=None):
        """shuffle_points: the sample's shuffle in front of the voxelizer (utils.py:35).
          True / "host": np.random.shuffle of the sample's cloud on the host, in place like the reference; False: none.
          "index":  shuffle.draw_index at that place — the sample's first draw, the same np.random draws — the cloud is
                    uploaded as read and `vn_permute_points` gathers the rows right behind the copy, in front of the crop,
                    the paste and the augmentation: voxel buffers, labels and the np.random state after the batch are
                    those of True, bit for bit.
          "device": shuffle.draw_keys at that place (one randint of six uint32), then `vn_shuffle_points`: a keyed
                    bijection evaluated per thread, no host work proportional to the cloud.  Another shuffle than the
                    reference's, and other np.random consumption.
          Anything else raises ValueError.  Divergence of the two device modes: the caller's `pcl` array is NOT modified,
          and the batch's raw-lidar element (element 6) is the cloud AS READ, not the shuffled one.
        augment: the reference's pcl_augmentation (dataset.py:122-219) per sample — drawn from np.random after the
        sample's shuffle, applied to the (cropped) cloud on the device in front of the voxelizer; the batch's `label`
        element then holds the MOVED label lines (augment.augment_labels), its raw-lidar element the host cloud as shuffled.
        An `augment.ComposeRecipe` instance instead of True: the composed recipe (object noise, flip, rotation, scaling,
        translation for EVERY sample — augment.draw_compose / compose_labels / vn_augment_compose), drawn and launched at
        the same two places.  True and False are exactly what they were; anything else raises ValueError.
        fov_calib_dir: RAW sweeps — crop every cloud to the camera field of view on the device before it is voxelized
        (the reference does this offline, preprocess_data.py:42-154, and trains on the rewritten .bin files):
        `<fov_calib_dir>/<tag>.txt` is the sample's KITTI object calibration file, the image size is the sample's image's
        (or image_shape when images are not loaded).  The crop keeps the input order, so shuffling the raw cloud first
        still hands the voxelizer a uniformly shuffled cropped cloud.
        gt_sampler: a gtsample.GTSampler — per sample, after the shuffle and before the augmentation's draw,
        `gt_sampler.draw(labels, tag)` picks database objects that collide with nothing in the frame; their points are
        pasted into the (cropped) cloud on the device in front of the augmentation (the scene points inside their boxes
        go) and the batch's `label` element holds labels + their lines (moved by the augmentation when it is on).  None:
        nothing is drawn, nothing is launched.  A sampler with a `visibility` pastes with vn_gt_paste_visible: the
        augmentation's draw still runs on labels + the lines of EVERY candidate (a rejected object still takes part in
        its collision test), and `concat` removes the rejected objects' lines from the sample's (moved) labels.
        part_augment: a part_augment.PartRecipe — per sample, after the sampler's draw and before the augmentation's,
        `part_augment.draw_parts` runs on the labels including the pasted lines; `vn_part_augment` then works on the cloud in
        place, behind the paste and in front of the augmentation (pyramids of objects dropped, thinned, swapped between
        objects of a class).  The label lines are unchanged.  With a visibility sampler
        the paste's device-side visible counts gate the pasted objects' entries: a rejected object owns no point and is
        nobody's partner.  None: nothing is drawn, nothing is launched; anything else raises ValueError."""
        # (strings are truthy: an unknown one must not fall through to the host shuffle)
        if isinstance(shuffle_points, str) and shuffle_points in ("host", "index", "device"):
            self._shuffle_mode = shuffle_points
        elif isinstance(shuffle_points, (bool, np.bool_, int)) and shuffle_points in (True, False):
            self._shuffle_mode = "host" if shuffle_points else None
        else:
            raise ValueError(f"shuffle_points={shuffle_points!r}: expected True, False, 'host', 'index' or 'device'")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.VoxelnetHipError("DeviceCollate needs a HIP device (no CPU path)")
        self.grid = grid_config("Car" if target == "Car" else "Pedestrian")    # utils.py:24-33 ('Car' else ped/cyc)
        self.shuffle_points = shuffle_points
        self.fov_calib_dir, self.image_shape = fov_calib_dir, tuple(image_shape)
        self.recipe = None
        if isinstance(augment, (bool, np.bool_)):
            self.augment = bool(augment)
        else:
            from .augment import ComposeRecipe
            if not isinstance(augment, ComposeRecipe):
                raise ValueError(f"augment={augment!r}: expected True, False or an augment.ComposeRecipe")
            self.augment, self.recipe = False, augment
        self.gt_sampler = gt_sampler
        if part_augment is not None:
            from .part_augment import PartRecipe
            if not isinstance(part_augment, PartRecipe):
                raise ValueError(f"part_augment={part_augment!r}: expected None or a part_augment.PartRecipe")
        self.part_augment = part_augment
        self.stream = pipeline_stream(self.device)      # (shared with the target generator: see voxelize.pipeline_stream)

    def launch(self, parts):
        """enqueue the copies and the voxelization of one batch on the pipeline's stream; returns a handle"""
        handles = []
        if self.augment or self.recipe is not None:
            from . import augment as A
        visibility = None
        if self.gt_sampler is not None:
            from . import gtsample as G
            visibility = getattr(self.gt_sampler, "visibility", None)
        if self.part_augment is not None:
            from . import part_augment as PA
        if self.augment or self.recipe is not None or self.gt_sampler is not None:
            parts = list(parts)
        mode = self._shuffle_mode
        if mode in ("index", "device"):
            from . import shuffle as S
        with torch.cuda.stream(self.stream):
            for b, p in enumerate(parts):
                pcl = p[2]
                if mode == "host":
                    np.random.shuffle(pcl)                                     # utils.py:35, in place like the reference
                elif mode == "index":
                    perm = S.draw_index(pcl.shape[0])                          # the same draws; the rows move on the device
                elif mode == "device":
                    perm = S.draw_keys()
                pasted = None
                if self.gt_sampler is not None:
                    pasted = self.gt_sampler.draw(p[3], p[0])                  # host: O(boxes); no points yet
                    if pasted.lines:
                        p = parts[b] = (p[0], p[1], p[2], list(p[3]) + pasted.lines, *p[4:])
                    else:
                        pasted = None                                          # nothing accepted: no launch, the cloud passes
                if self.part_augment is not None:
                    part_params = PA.draw_parts(p[3], self.part_augment)       # host: O(boxes); the lines stay as they are
                if self.augment:
                    params = A.draw_augmentation(p[3])                         # dataset.py:122-219, host: O(boxes)
                    parts[b] = (p[0], p[1], p[2], A.augment_labels(p[3], params), *p[4:])
                    assert len(parts[b][3]) == len(p[3])                       # one line per input line, in order
                elif self.recipe is not None:
                    params = A.draw_compose(p[3], self.recipe)                 # the composed recipe, host: O(boxes^2)
                    parts[b] = (p[0], p[1], p[2], A.compose_labels(p[3], params), *p[4:])
                    assert len(parts[b][3]) == len(p[3])
                host = torch.from_numpy(np.ascontiguousarray(pcl[:, :4], dtype=np.float32)).pin_memory()
                pts = host.to(self.device, non_blocking=True)
                if mode == "index":
                    # right behind the copy on this stream; `keep` = the staged index table, referenced by the handle
                    # until the batch is consumed, like `host`
                    pts, keep = S.enqueue_permute_points(pts, perm)
                    host = (host, keep)
                elif mode == "device":
                    pts, keep = S.enqueue_shuffle_points(pts, perm)
                    host = (host, keep)
                if self.fov_calib_dir is not None:
                    from .fov import fov_crop_device, load_calib
                    P, Tr, R = load_calib(os.path.join(self.fov_calib_dir, str(p[0]) + ".txt"))
                    rows, cols = p[1].shape[:2] if p[1] is not None else self.image_shape
                    # padded form: no 4-byte read-back per sample (it would stall the host behind everything queued
                    # on this stream); the rows past the device-side count are NaN points, which the voxelizer drops
                    pts, _ = fov_crop_device(pts, P, Tr, R, rows, cols, padded=True)
                rejects = None
                if pasted is not None and visibility is not None:
                    # the same place; the visible counts follow in pinned memory (concat reads them): the sample's last
                    # len(pasted.lines) label lines are pasted ones
                    pts, keep, visible, pasted_result = G.enqueue_gt_paste_visible(pts, pasted, visibility, return_result=True)
                    host = (host, keep)
                    rejects = (visible, len(pasted.lines), visibility.min_visible)
                elif pasted is not None:
                    # behind the copy / the crop on this stream; the NaN rows of the padded crop go, NaN rows come out, so
                    # the count is not read back either; `keep` = the staged table and object points
                    pts, keep = G.enqueue_gt_paste(pts, pasted)
                    host = (host, keep)
                if self.part_augment is not None:
                    # in place, behind the paste on this stream; the entries of the pasted lines (the table's last ones) are
                    # gated by the visible counts where they are, on the device: nothing is read back
                    gate = {}
                    if rejects is not None:
                        gate = dict(gate=pasted_result.visible_device, gate_first=len(part_params.table) - len(pasted.lines),
                                    gate_min=visibility.min_visible)
                    pts, keep, _ = PA.enqueue_part_points(pts, part_params, out=pts, **gate)
                    host = (host, keep)
                if self.augment:
                    # in place, behind the copy / the crop on this stream; `keep` = the staged box table, referenced
                    # by the handle until the batch is consumed, like `host`
                    pts, keep = A.enqueue_augment_points(pts, params, out=pts)
                    host = (host, keep)
                elif self.recipe is not None:
                    pts, keep = A.enqueue_compose_points(pts, params, out=pts)          # the same place, one launch
                    host = (host, keep)
                handles.append((voxelize_device_async(pts, self.grid, b, coord_cols=4), pts, host, rejects))
        return parts, handles

    def concat(self, launched):
        """second stage, still on the pipeline's stream: slice the capacity-sized outputs to K and make the concatenations
        the model starts with (RPN3D.detect) — off the train step's dependency chain.  `DeviceBatcher` calls this for
        batch i BEFORE it launches batch i+1, so the concatenation of batch i is queued behind batch i's own voxelizer
        only (queued behind the next batch's copies, crop and voxelization it would make step i wait for all of them).
        With a visibility sampler this is also where the label lines of the objects the device rejected go: the counts
        were copied to pinned memory in front of the sample's voxelizer, whose result is waited for here anyway."""
        if len(launched) == 5:
            return launched
        parts, handles = launched
        feats, nums, coords = [], [], []
        for b, (h, _, _, rejects) in enumerate(handles):
            f, c, n = h.result()                    # waits for the 4-byte K copy of this sample only
            if rejects is not None:
                # everything queued earlier on the pipeline's stream has run: the pinned counts are there
                visible, n_pasted, min_visible = rejects
                p = parts[b]
                parts[b] = (p[0], p[1], p[2], drop_rejected_lines(p[3], n_pasted, visible.numpy(), min_visible), *p[4:])
            feats.append(f)
            coords.append(c)
            nums.append(n)
        if handles:
            feats = VoxelBatch.ahead(feats, self.stream, torch.float32)
            coords = VoxelBatch.ahead(coords, self.stream, torch.int64)
        return parts, handles, feats, nums, coords

    def finish(self, launched):
        parts, handles, feats, nums, coords = self.concat(launched)
        if handles:
            torch.cuda.current_stream().wait_event(handles[-1][0].event)       # consumer stream after the voxelizer
            for t in list(feats) + list(coords) + nums:
                t.record_stream(torch.cuda.current_stream())
        return ([p[0] for p in parts], np.array([p[3] for p in parts] + [None], dtype=object)[:-1], feats, nums, coords,
                np.array([p[1] for p in parts] + [None], dtype=object)[:-1],
                np.array([p[2] for p in parts] + [None], dtype=object)[:-1])

    def __call__(self, parts):
        return self.finish(self.launch(parts))


class DeviceBatcher:
    """Iterate an iterable of `parts` lists (e.g. DataLoader(ds, batch_size, collate_fn=list, num_workers=8)) as
    device-resident 7-tuples, one batch ahead: while the model trains on batch i, batch i+1 is being copied and
    voxelized on the pipeline's own stream."""

    def __init__(self, loader, device="cuda:0", target="Car", shuffle_points=True, fov_calib_dir=None, image_shape=(375, 1242),
                 augment=False, gt_sampler=None, part_augment=None):
        self.loader = loader
        self.collate = DeviceCollate(device, target, shuffle_points, fov_calib_dir, image_shape, augment, gt_sampler=gt_sampler,
                                     part_augment=part_augment)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        it = iter(self.loader)
        pending = None
        for parts in it:
            if pending is not None:
                pending = self.collate.concat(pending)     # batch i's concatenation in front of batch i+1's pipeline work
            launched = self.collate.launch(parts)
            if pending is not None:
                yield self.collate.finish(pending)
            pending = launched
        if pending is not None:
            yield self.collate.finish(pending)
