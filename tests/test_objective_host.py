"""CPU: what tests/test_gpu_objective.py's gradient bar can see, established on the reference alone (tests/objective_ref.py).

The GPU test holds all 108 gradients of the composed objective — focal + sine + 2 DIoU + dir_weight L_dir + 1 L_iou_head — to
OBJECTIVE_BAR relative L2 of the frozen-mask float64 oracle.  Here, on the same tiny golden batch and with the very head
weights the GPU test's model has (torch.manual_seed(7) before RPN3D is constructed on the host), the reference with ONE term
left out is compared with the full reference: if the smallest relative L2 distance over every trunk and VFE parameter is at
least 3 x OBJECTIVE_BAR for each of the five terms, a backward that loses (or doubles: the distance is the same) any one
term's contribution to any one parameter misses the GPU test's bar by a factor of three or more.  No device code is
involved, and none is edited to show that the GPU test can fail.

The four heads' own parameters are left out of the minimum: a head's gradient does not depend on the other terms at all
(prob_conv's does not change when the direction head goes), which is why the one-head tests cannot see the composition."""
import pytest
import torch

import objective_ref as O

# the direction head at RPN3D's default weight; the condition below decides whether the GPU test can keep it
DIR_WEIGHT = O.MODEL_KW["dir_weight"]


def host_head_params():
    """the two site heads' parameters as tests/test_gpu_objective.py's model has them: RPN3D's own initialisation under
    torch.manual_seed(7), drawn on the host (the GPU test constructs on the host and moves the module)"""
    from voxelnet_amd import model as M
    torch.manual_seed(7)
    m = M.RPN3D("Car", **O.MODEL_KW)
    p = dict(m.named_parameters())
    return {k: p[k].detach().clone() for k in O.HEAD_KEYS}


@pytest.fixture(scope="module")
def leave_one_out(golden):
    """one float64 forward of the oracle (plain ReLU), six backward passes: the full objective and each term dropped"""
    feats, coords, targets = O.tiny_batch(golden)
    prob, reg, z_dir, z_iou, leaves = O.oracle_run(feats, coords, host_head_params())
    keys = [k for k in leaves if k not in O.HEAD_KEYS and "prob_conv" not in k and "reg_conv" not in k and not O.bn_fronted_bias(k)]
    zero_keys = [k for k in leaves if O.bn_fronted_bias(k)]
    res = {}
    for drop in (None,) + O.TERMS:
        o = O.objective(prob, reg, z_dir, z_iou, *targets, O.ANCHORS_TINY, **_switches(), drop=drop, guard=drop is None)
        grads = torch.autograd.grad(o["total"], [leaves[k] for k in keys + zero_keys], retain_graph=True)
        res[drop] = (o, dict(zip(keys + zero_keys, grads)))
    return keys, zero_keys, res


def _values(o):
    """objective()'s result with every tensor as a Python float"""
    f = lambda v: float(v.detach()) if torch.is_tensor(v) else v          # noqa: E731
    return {k: ({n: f(x) for n, x in v.items()} if k == "terms" else f(v)) for k, v in o.items()}


def _switches():
    kw = {k: v for k, v in O.MODEL_KW.items() if k not in ("dir_head", "iou_head")}
    return dict(kw, dir_weight=DIR_WEIGHT)


def test_every_term_moves_every_trunk_gradient_by_three_bars(leave_one_out):
    keys, zero_keys, res = leave_one_out
    full = res[None][1]
    assert len(keys) == 104 - 4 - 23 and len(zero_keys) == 23          # 23 layers' conv / deconv biases sit in front of a BatchNorm
    for k in keys:
        assert float(full[k].norm()) > 0, k
    for k in zero_keys:                                                  # the true gradient: zero up to float64 rounding
        assert float(full[k].abs().max()) < 1e-9, k
    minima = {}
    for drop in O.TERMS:
        g = res[drop][1]
        d = {k: float((g[k] - full[k]).norm() / full[k].norm()) for k in keys}
        worst = min(d, key=d.get)
        minima[drop] = d[worst]
        shown = ", ".join(f"{k.split('.', 1)[1]} {d[k]:.2e}" for k in ("middle_rpn.deconv3.deconv.weight", "middle_rpn.block1.0.conv.weight",
                                                                          "middle_rpn.middle_layer.0.conv.weight", "feature_net.vfe_1.fcn.0.weight"))
        print(f"without {drop:8s}: smallest relative L2 change {d[worst]:.2e} ({worst}); {shown}")
    print("leave-one-out minima (dir, iou_head, iou, focal, sin):", " ".join(f"{minima[t]:.2e}" for t in O.TERMS),
          f"; bar {O.OBJECTIVE_BAR:.1e}, dir_weight {DIR_WEIGHT}")
    for drop in O.TERMS:
        assert minima[drop] >= 3 * O.OBJECTIVE_BAR, (drop, minima[drop])


def test_guards_and_all_five_terms_are_positive(leave_one_out):
    _, _, res = leave_one_out
    o = _values(res[None][0])
    g = o["guards"]
    t = o["terms"]
    print("guards:", g, "; terms:", t, f"mean IoU {o['mean_iou']:.4f}")
    assert g["edge_gap"] > 1e-6 and g["min_logit"] > 1e-6 and g["n_pairs"] == 33 and g["targets_above_0"] >= 1
    for k, v in t.items():
        assert v is not None and v > 0, k
    # the composition: which scalar each term joins
    kw = _switches()
    extra_cls = kw["dir_weight"] * t["dir"] + kw["iou_head_weight"] * t["iou_head"]
    assert float(o["cls_loss"]) == pytest.approx(t["focal"] + extra_cls, rel=1e-12)
    assert float(o["reg_loss"]) == pytest.approx(t["sin"] + kw["iou_weight"] * t["iou"], rel=1e-12)
    assert float(o["loss"]) == pytest.approx(float(o["cls_loss"]) + float(o["reg_loss"]), rel=1e-12)
    assert t["focal"] == pytest.approx(O.ABS[0] * float(o["cls_pos"]) + O.ABS[1] * float(o["cls_neg"]), rel=1e-12)
    # a dropped term is gone from the value too, and only that one
    for drop in ("dir", "iou_head", "iou"):
        od = _values(res[drop][0])
        assert od["terms"][drop] is None
        w = {"dir": kw["dir_weight"], "iou_head": kw["iou_head_weight"], "iou": kw["iou_weight"]}[drop]
        assert float(od["loss"]) == pytest.approx(float(o["loss"]) - w * t[drop], rel=1e-12)
    no_focal, no_sin = _values(res["focal"][0]), _values(res["sin"][0])
    assert no_focal["cls_loss"] != o["cls_loss"] and no_focal["reg_loss"] == o["reg_loss"]
    assert no_sin["reg_loss"] != o["reg_loss"] and no_sin["cls_loss"] == o["cls_loss"]


def test_host_head_weights_are_the_constructors(leave_one_out):
    """the draw is reproducible and is RPN3D's initialisation: the IoU-aware head's bias starts at 0, nothing else does"""
    a, b = host_head_params(), host_head_params()
    assert all(torch.equal(a[k], b[k]) for k in O.HEAD_KEYS)
    assert tuple(a[O.HEAD_KEYS[0]].shape) == tuple(a[O.HEAD_KEYS[2]].shape) == (2, 768, 1, 1)
    assert not a[O.HEAD_KEYS[3]].any() and a[O.HEAD_KEYS[1]].abs().min() > 0
    assert not torch.equal(a[O.HEAD_KEYS[0]], a[O.HEAD_KEYS[2]])
