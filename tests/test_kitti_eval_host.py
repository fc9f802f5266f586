"""CPU: the host side of the image-plane scoring — tests/kitti_ref.py against closed forms, and
voxelnet_amd/evaluate.py's label parsing, AOS arithmetic, result lines and calibration readers against it."""
import math
import os

import numpy as np
import pytest

import kitti_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB_TEXT = """P0: 7.215377e+02 0.0 6.095593e+02 0.0 0.0 7.215377e+02 1.728540e+02 0.0 0.0 0.0 1.0 0.0
P1: 7.215377e+02 0.0 6.095593e+02 -3.875744e+02 0.0 7.215377e+02 1.728540e+02 0.0 0.0 0.0 1.0 0.0
P2: 7.215377000000e+02 0.0 6.095593000000e+02 4.485728000000e+01 0.0 7.215377e+02 1.728540e+02 2.163791e-01 0.0 0.0 1.0 2.745884e-03
P3: 7.215377e+02 0.0 6.095593e+02 -3.395242e+02 0.0 7.215377e+02 1.728540e+02 2.199936e+00 0.0 0.0 1.0 2.729905e-03
R0_rect: 9.999239e-01 9.837760e-03 -7.445048e-03 -9.869795e-03 9.999421e-01 -4.278459e-03 7.402527e-03 4.351614e-03 9.999631e-01
Tr_velo_to_cam: 7.533745e-03 -9.999714e-01 -6.166020e-04 -4.069766e-03 1.480249e-02 7.280733e-04 -9.998902e-01 -7.631618e-02 9.998621e-01 7.523790e-03 1.480755e-02 -2.717806e-01
Tr_imu_to_velo: 9.999976e-01 7.553071e-04 -2.035826e-03 -8.086759e-01 -7.854027e-04 9.998898e-01 -1.482298e-02 3.195559e-01 2.024406e-03 1.482454e-02 9.998881e-01 -7.997231e-01
"""


# ------------------------------------------------------------------------------- the reference against closed forms
def test_reference_box_on_the_optical_axis():
    """identity extrinsics up to the axis permutation (camera x = -lidar y, y = -lidar z, z = lidar x), principal point in
    the image centre: a box on the optical axis, heading along it, has a 2D box symmetric about the principal point's
    column, alpha = ry, and the closed-form pinhole extents"""
    Tr = np.array([[0.0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]])
    f, cu, cv = 700.0, 620.5, 187.0
    P2 = np.array([[f, 0, cu, 0], [0, f, cv, 0], [0, 0, 1, 0.0]])
    calib = (P2, Tr, np.eye(4))
    x, z, h, w, l = 20.0, -1.0, 1.5, 1.6, 4.0
    for r in (0.0, math.pi / 2, -math.pi / 2):
        p = K.project_box([x, 0.0, z, h, w, l, r], calib)
        al, x1, y1, x2, y2 = p["row"][:5]
        assert p["on"] and abs((x1 + x2) / 2 - cu) < 1e-9
        assert abs(al - p["row"][11]) < 1e-12 and abs(p["row"][11] - K.wrap(-r - math.pi / 2)) < 1e-15
        ext, depth = (w, l) if r == 0.0 else (l, w)          # across the axis, along it
        near = x - depth / 2
        assert abs(x1 - (cu - f * ext / 2 / near)) < 1e-9 and abs(x2 - (cu + f * ext / 2 / near)) < 1e-9
        assert abs(y2 - (cv + f * (-z) / near)) < 1e-9 and abs(y1 - (cv - f * (z + h) / near)) < 1e-9
        assert np.allclose(p["row"][5:11], [h, w, l, 0.0, -z, x], atol=1e-12)
    # the issue's figures, with the mean calibration: a 1.5-m-high car
    car = lambda x, y, z: K.project_box([x, y, z, 1.5, 1.6, 3.9, 0.0])      # noqa: E731
    a, b = car(20, 0, -1.7), car(60, 10, -1.5)
    assert a["on"] and round(a["row"][4] - a["row"][2]) == 62 and b["on"] and round(b["row"][4] - b["row"][2]) == 19
    assert not car(1.5, 0, -1.7)["on"] and not car(30, 35, -1.7)["on"]
    assert (car(1.5, 0, -1.7)["row"][1:5] == 0).all() and car(1.5, 0, -1.7)["depths"].min() < 0.1


def test_reference_round_trip_and_wrap():
    rng = np.random.default_rng(0)
    for _ in range(20):
        calib = K.perturbed_calib(rng)
        box = [rng.uniform(5, 60), rng.uniform(-20, 20), rng.uniform(-2, -1), 1.5, 1.6, 4.0, rng.uniform(-3.1, 3.1)]
        line = K.label_line("Car", box, calib, digits=12)
        back = K.frame_ground_truth([line], "Car", K.DIFFS, calib)["boxes"][0]
        assert np.abs(back - np.array(box)).max() < 1e-9
    assert K.wrap(math.pi) == math.pi and K.wrap(-math.pi) == math.pi and abs(K.wrap(3 * math.pi / 2) + math.pi / 2) < 1e-15
    assert K.seam_distance(math.pi) == 0 and abs(K.seam_distance(-math.pi + 0.25) - 0.25) < 1e-12
    assert K.iou_2d([0, 0, 2, 2], [1, 0, 3, 2]) == 1 / 3 and K.iou_2d([0, 0, 0, 0], [0, 0, 0, 0]) == 0
    assert K.dontcare_overlap([0, 0, 10, 10], [[5, 0, 20, 10], [0, 0, 4, 10]]) == 0.5


def test_mean_calibration_is_the_projects():
    from voxelnet_amd import evaluate as E
    from voxelnet_amd import targets as T
    P = np.load(os.path.join(ROOT, "tests", "golden", "fov_crop.npz"))["P"].astype(np.float64)
    P2, Tr, R0 = E.mean_calib()
    assert np.array_equal(P2, P) and np.array_equal(K.MEAN_P2, P)
    assert np.array_equal(Tr, T._T_VELO_2_CAM) and np.array_equal(R0, T._R_RECT_0)
    assert np.array_equal(K.MEAN_TR, Tr) and np.array_equal(K.MEAN_R0, R0)
    row, full = E._calib_rows(None)
    assert np.array_equal(row[:12].reshape(3, 4), (R0 @ Tr)[:3]) and np.array_equal(row[12:].reshape(3, 4), P)


# ------------------------------------------------------------------------------------------------ label parsing
def _lines():
    car = [20.0, 3.0, -1.6, 1.5, 1.6, 4.0, 0.2]
    return [
        K.label_line("Car", car, trunc=0.0, occ=0, bbox=[100, 100, 200, 145], alpha=-1.2),          # valid everywhere
        K.dontcare_line([500.0, 150.0, 560.0, 180.0]),
        K.label_line("Car", car, trunc=0.2, occ=1, bbox=[100, 100, 200, 130]),                      # not easy
        K.label_line("Van", car, bbox=[1, 2, 3, 4]),
        K.label_line("Car", car, trunc=0.6, occ=0, bbox=[100, 100, 200, 160]),                      # too truncated
        K.label_line("Person_sitting", car), K.label_line("Pedestrian", car), K.label_line("Cyclist", car),
        K.label_line("Car", car, occ=2, bbox=[100, 100, 200, 124.99]),                              # under 25 px
        K.dontcare_line([0.0, 10.5, 60.25, 80.0]), K.label_line("Tram", car), K.label_line("Misc", car),
    ]


@pytest.mark.parametrize("cls,n,flags", [
    ("Car", 5, [[0, 0, 1, 0, 0], [0, 1, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 1, 1, 1]]),
    ("Pedestrian", 2, [[1, 0]] * 4), ("Cyclist", 1, [[0]] * 4)])
def test_label_parsing(cls, n, flags):
    from voxelnet_amd import evaluate as E
    rng = np.random.default_rng(1)
    calib = K.perturbed_calib(rng)
    lines = _lines()
    got, n_valid = E.kitti_ground_truth([lines, []], cls, K.DIFFS, [calib, None])
    ref = K.frame_ground_truth(lines, cls, K.DIFFS, calib)
    assert got["boxes"][0].shape == (n, 7) and np.abs(got["boxes"][0] - ref["boxes"]).max() < 1e-12
    assert got["flags"][0].tolist() == flags and np.array_equal(got["flags"][0] != 0, ref["flags"])
    assert np.array_equal(got["bbox"][0], ref["bbox"]) and np.array_equal(got["alpha"][0], ref["alpha"])
    assert got["dontcare"][0].tolist() == [[500.0, 150.0, 560.0, 180.0], [0.0, 10.5, 60.25, 80.0]]
    assert np.array_equal(got["dontcare"][0], ref["dontcare"])
    assert n_valid[0].tolist() == [int(sum(1 for v in row if v == 0)) for row in flags] and n_valid[1].tolist() == [0] * 4
    assert got["boxes"][1].shape == (0, 7) and got["flags"][1].shape == (4, 0) and got["dontcare"][1].shape == (0, 4)
    if cls == "Car":
        assert got["bbox"][0][0].tolist() == [100, 100, 200, 145] and got["alpha"][0][0] == -1.2
        assert got["bbox"][0][2].tolist() == [1, 2, 3, 4]          # the Van: ignored everywhere, third kept line
        # the frame's own calibration is used, and there is no 5-degree snap: a heading 2 degrees off -pi/2 stays
        mean = E.kitti_ground_truth([lines], cls, K.DIFFS, None)[0]["boxes"][0]
        assert np.abs(mean[:, :3] - got["boxes"][0][:, :3]).max() > 0.05
        snap = K.label_line("Car", [20.0, 3.0, -1.6, 1.5, 1.6, 4.0, -math.pi / 2 + 0.035], digits=6)
        r = E.kitti_ground_truth([[snap]], "Car")[0]["boxes"][0][0, 6]
        assert abs(r - (-math.pi / 2 + 0.035)) < 1e-5
    assert E.NEIGHBOUR_CLASSES == K.NEIGHBOURS and E.CLASS_CFG["Car"]["accept"] == ("Car", "Van")


# -------------------------------------------------------------------------------------------------------- AOS
def _pool(seed, n=60):
    rng = np.random.default_rng(seed)
    scores = rng.permutation(n).astype(np.float64) / n
    status = rng.choice([1, 0, -1], size=n, p=[0.5, 0.3, 0.2])
    return scores, status, int((status == 1).sum()) + 7


@pytest.mark.parametrize("recall_points", [40, 11])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_aos_arithmetic(seed, recall_points):
    from voxelnet_amd import evaluate as E
    scores, status, n_gt = _pool(seed)
    ap = E.average_precision(scores, status, n_gt, recall_points)
    tp = status == 1
    aos = lambda delta: E.average_orientation_similarity(                                            # noqa: E731
        scores, status, np.where(tp, (1 + np.cos(delta)) / 2, 0.0), n_gt, recall_points)
    assert 0 < ap < 1
    assert aos(np.zeros(len(status))) == ap                           # every similarity 1
    assert abs(aos(np.full(len(status), math.pi / 2)) - 0.5 * ap) < 1e-15
    assert abs(aos(np.full(len(status), math.pi))) < 1e-15
    rng = np.random.default_rng(seed + 10)
    delta = rng.uniform(-math.pi, math.pi, len(status))
    mixed = aos(delta)
    assert 0 < mixed < ap
    ref_ap, ref_aos = K.ap_and_aos(scores, status, np.where(tp, (1 + np.cos(delta)) / 2, 0.0), n_gt, recall_points)
    assert abs(ref_ap - ap) < 1e-12 and abs(ref_aos - mixed) < 1e-12
    assert math.isnan(E.average_orientation_similarity(scores, status, np.zeros(len(status)), 0))
    assert E.average_orientation_similarity([], [], [], 5) == 0.0


# ------------------------------------------------------------------------------------------------ result lines
def test_result_lines_parse_back():
    from voxelnet_amd import evaluate as E
    from voxelnet_amd.targets import label_to_gt_box_3d
    rng = np.random.default_rng(4)
    for _ in range(10):
        box = np.array([rng.uniform(8, 60), rng.uniform(-5, 5), rng.uniform(-2, -1), 1.52, 1.63, 3.88, rng.uniform(-1.4, 1.4)])
        p = K.project_box(box)
        assert p["on"]
        line = E.format_result_line("Car", p["row"], 0.87654)
        assert line == K.result_line("Car", p["row"], 0.87654)
        f = line.split()
        assert len(f) == 16 and f[:3] == ["Car", "-1", "-1"] and f[15] == "0.8765"
        assert all(len(v.split(".")[1]) == 2 for v in f[3:15])
        back = label_to_gt_box_3d([[" ".join(f[:15])]], "Car", "lidar")[0][0]          # (mean calibration, as the line's)
        # two decimals: 0.005 per camera coordinate -> 0.005 * sqrt(3) in the lidar frame; sizes and heading 0.005
        assert np.abs(back[:3] - box[:3]).max() <= 0.005 * math.sqrt(3) + 1e-6
        assert np.abs(back[3:6] - box[3:6]).max() <= 0.005 + 1e-9
        assert abs(math.remainder(back[6] - box[6], math.pi)) <= 0.005 + 1e-9          # (label_to_gt_box_3d folds by pi)
        assert np.abs(np.array(f[4:8], dtype=float) - p["row"][1:5]).max() <= 0.005 + 1e-9


# ------------------------------------------------------------------------------------------- calibration files
def test_load_calib_default_is_unchanged_and_float64_readers(tmp_path):
    from voxelnet_amd import evaluate as E
    from voxelnet_amd import fov
    path = tmp_path / "000007.txt"
    path.write_text(CALIB_TEXT)
    P, Tr, R = fov.load_calib(str(path))
    assert P.dtype == Tr.dtype == R.dtype == np.float32 and P.shape == (3, 4) and Tr.shape == R.shape == (4, 4)
    rows = {l.split(":")[0]: np.array(l.split()[1:], dtype=np.float64) for l in CALIB_TEXT.strip().splitlines()}
    assert np.array_equal(P, rows["P2"].reshape(3, 4).astype(np.float32))
    assert np.array_equal(Tr[:3], rows["Tr_velo_to_cam"].reshape(3, 4).astype(np.float32)) and Tr[3].tolist() == [0, 0, 0, 1]
    assert np.array_equal(R[:3, :3], rows["R0_rect"].reshape(3, 3).astype(np.float32)) and R[3].tolist() == [0, 0, 0, 1]
    P64, Tr64, R64 = fov.load_calib(str(path), dtype=np.float64)
    assert P64.dtype == np.float64 and np.array_equal(P64, rows["P2"].reshape(3, 4))
    Pk, Trk, Rk = E.load_kitti_calib(str(path))
    assert np.array_equal(Pk, P64) and np.array_equal(Trk, Tr64) and np.array_equal(Rk, R64)
    src = E.calib_source(str(tmp_path))
    assert np.array_equal(src("000007")[0], P64) and E.calib_source("mean")("x") is None
    assert E.calib_source(lambda tag: tag)("t") == "t"
    with pytest.raises(ValueError):
        E.calib_source(3)


def test_evaluator_needs_a_device_and_the_library_checks_sizes():
    from voxelnet_amd import _lib
    from voxelnet_amd import evaluate as E
    with pytest.raises(_lib.VoxelnetHipError):
        E.KittiDetectionEvaluator("Car", "cpu")
    lib = _lib.load()
    EINVAL = -1
    b2i = lambda B, k: lib.vn_boxes_to_image(None, None, None, None, B, k, None, None, None)      # noqa: E731
    assert b2i(0, 20) == 0 and b2i(2, 20) == EINVAL and b2i(0, 33) == EINVAL and b2i(0, 0) == EINVAL and b2i(-1, 20) == EINVAL

    def mi(B, k, G, D, n):
        return lib.vn_eval_match_image(*([None] * 13), B, k, G, D, n, 0.7, 0.7, 0.7, None, None, None, None, None, 0, None)
    assert mi(0, 20, 12, 0, 4) == 0 and mi(0, 32, 128, 64, 8) == 0
    for bad in [(0, 33, 12, 0, 4), (0, 20, 129, 0, 4), (0, 20, 12, 65, 4), (0, 20, 12, -1, 4), (0, 20, 12, 0, 9), (0, 20, 0, 0, 4),
                (0, 0, 12, 0, 4), (0, 20, 12, 0, 0), (2, 20, 12, 0, 4)]:
        assert mi(*bad) == EINVAL, bad
    assert lib.vn_eval_match_image(*([None] * 13), 0, 20, 12, 0, 4, float("nan"), 0.7, 0.7, None, None, None, None, None, 0,
                                   None) == EINVAL
    assert (_lib.VN_EVAL_BBOX, _lib.VN_EVAL_MAX_DC, _lib.VN_EVAL_IMAGE_ROW) == (2, 64, 12)
