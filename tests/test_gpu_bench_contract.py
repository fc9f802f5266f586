"""GPU: bench.py's output contract.  The driver parses ONE JSON line of `python bench.py` (train.py:145-155 is the loop it
times; BASELINE.json names the metric and the workload); a refactor of bench.py must not silently drop a key the driver or
the judge reads.  conftest.py starts `bench.py --full --steps 2 --warmup 1 --force-reducer --dump-outputs DIR` (N = 1 with
the data-parallel bucket path attached) as its own process before this process touches the GPU; here its line is parsed
and the outputs it wrote are checked."""
import json
import os

import numpy as np
import pytest

from conftest import BENCH_RUN

pytestmark = pytest.mark.gpu


def test_bench_line_carries_the_keys_the_driver_reads():
    if "proc" not in BENCH_RUN:
        pytest.skip("bench.py was not started (not a `-m gpu` session, or VN_NO_DDP_REHEARSAL=1)")
    p = BENCH_RUN["proc"]
    try:
        rc = p.wait(timeout=900)
    except Exception:  # noqa: BLE001
        p.kill()
        rc = -9
    err = open(os.path.join(BENCH_RUN["dir"], "bench.err")).read()[-3000:]
    out = open(os.path.join(BENCH_RUN["dir"], "bench.json")).read().strip().splitlines()
    assert rc == 0 and out, f"bench.py exit {rc}\n{err}"
    d = json.loads(out[-1])
    # the driver's contract (one line, these keys)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["metric"].startswith("point-clouds/sec fwd+bwd, KITTI car voxel grid, batch=2")
    assert "BASELINE configs[1]" in d["config"]["workload"] and "model" not in d["config"]
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["data"] == "synthetic" and d["vs_baseline"] is None and d["value"] > 0
    # the tier's two objects
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "mfma" and 0.0 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is None or r["traffic"] > 0
    assert "traffic_source" in r                                   # says where `traffic` comes from, or why it is null
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0
    # the data-parallel path at world size 1 (--force-reducer): the fields the first SCALE run will be read by
    a = d["allreduce"]
    assert a["exposed_ms_per_step"] is not None and a["exposed_ms_per_step"] >= 0.0
    assert len(a["bucket_bytes"]) == 5 and sum(a["bucket_bytes"]) == 4 * 6809392
    assert a["comm_stream"] in ("private",) or a["comm_stream"].startswith("pipeline")
    assert "library" in d and "build" in d["library"] and "host_enqueue_ms_per_step" in d
    # --dump-outputs: what the last timed step returned and the model state it left, float32 / float64, <= 64 MB in all
    od = os.path.join(BENCH_RUN["dir"], "outputs")
    names = sorted(os.listdir(od))
    for n in ("prob", "reg", "loss", "cls_loss", "reg_loss", "cls_pos_loss", "cls_neg_loss", "param.middle_rpn.block3.0.conv.weight",
              "param.middle_rpn.block3.0.batch_norm.running_var", "param.feature_net.vfe_1.fcn.0.bias"):
        assert n + ".npy" in names, n
    assert sum(os.path.getsize(os.path.join(od, n)) for n in names) <= 64e6
    for n in names:
        a = np.load(os.path.join(od, n))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
    assert np.load(os.path.join(od, "prob.npy")).shape == (2, 2, 200, 176)
    assert np.load(os.path.join(od, "reg.npy")).shape == (2, 14, 200, 176)
    assert float(np.load(os.path.join(od, "loss.npy"))) > 0
