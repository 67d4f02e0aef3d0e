"""Driver-contract test: bench.py emits one valid JSON line with the
required fields, on CPU, within a bounded time."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*extra):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--steps", "2", "--warmup", "1", "--pods-per-step", "4", *extra],
        capture_output=True, text=True, timeout=240, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    return json.loads(line)


def test_bench_json_contract():
    d = _run_bench("--full")
    assert d["metric"] == "Allocate() p50 latency"
    assert d["unit"] == "us"
    assert d["higher_is_better"] is False
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert d["vs_baseline"] is None
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    cfg = d["config"]
    for key in ("model", "gpus_per_pod", "discovered_gpus",
                "admission_p50_us", "rpc_floor_us", "pods_per_s_total"):
        assert key in cfg, key
    assert cfg["discovered_gpus"] == 8


def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain run (no --full) keeps the headline fields, skips the side
    measurements, and --dump-outputs writes the last step's RPC results,
    identical from run to run."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        out_dir = tmp_path / name
        d = _run_bench("--gpus", "2", "--dump-outputs", str(out_dir))
        assert d["metric"] == "Allocate() p50 latency"
        assert d["unit"] == "us" and d["dtype"] == "n/a"
        assert d["higher_is_better"] is False
        assert d["steps"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
        assert "rpc_floor_us" not in d["config"]
        assert "gpu_probe" not in d["config"]
        assert sorted(p.name for p in out_dir.iterdir()) == [
            "allocate_response_bytes.npy", "picked_device_ids.npy"]
        dumps.append({p.name: np.load(p) for p in out_dir.iterdir()})

    ids = dumps[0]["picked_device_ids.npy"]
    raw = dumps[0]["allocate_response_bytes.npy"]
    assert ids.dtype == np.float64 and ids.shape == (4, 2)
    assert set(ids.ravel()) <= {70.0 + i for i in range(8)}
    assert raw.dtype == np.float32 and raw.shape[0] == 4 and raw.shape[1] > 0

    # the dumped bytes are the AllocateResponse the caller received
    from kata_xpu_device_plugin_amd.plugin import api
    row = raw[0]
    resp = api.AllocateResponse.FromString(
        row[row >= 0].astype(np.uint8).tobytes())
    assert len(resp.container_responses[0].cdi_devices) == 2

    for name, arr in dumps[0].items():
        assert np.array_equal(arr, dumps[1][name]), name
