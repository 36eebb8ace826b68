"""bench.py's output contract (the driver parses this line every round).

One short run on the GPU at a small canvas: exactly one JSON line with the
metric, the whole-job value, the roofline object and the CPU baseline, and a
ray count that matches the reference's semantics for three_sphere (every
pixel hits a wall or the floor: one primary and one shadow ray per pixel).
Those runs pass --full; a plain run prints the headline figures alone and,
with --dump-outputs, writes the last timed frame.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline"}


def _run(*args, timeout=240):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_parses_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0 and "--gpus" in r.stdout and "--steps" in r.stdout
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_bench_line_contract():
    d = _run("--full", "--steps", "20", "--warmup", "2", "--width", "320", "--height", "240",
             "--cpu-seconds", "0.2")
    assert KEYS <= set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["unit"] == "Mray/s" and d["dtype"] == "f32" and d["scaling"] == "weak"
    assert d["config"]["rays_per_frame"] == 2 * 320 * 240
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # frames in flight (three contexts alternating) and one frame's own device time
    assert d["frames_in_flight"] == 3 and d["frame_latency_ms"] > 0
    assert d["frame_latency_ms"] == d["roofline"]["kernel_ms"]
    rl = d["roofline"]
    assert rl["unit"] == "TFLOP/s" and rl["peak"] == 157.3 and 0 < rl["frac"] < 1
    assert abs(rl["frac"] - rl["achieved"] / rl["peak"]) < 1e-12
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0
    s0 = cb["configs0_serial"]  # BASELINE configs[0]: Camera::render at 320x240, one thread
    assert s0["cores"] == 1 and s0["ms_per_frame"] > 0 and s0["rays_per_frame"] == 2 * 320 * 240
    # rays by kind and per generation
    assert d["rays_by_kind"] == {"primary": 320 * 240, "shadow": 320 * 240, "reflect": 0, "refract": 0}
    g = d["rays_by_generation"]
    assert g["traced"][0] == g["shaded"][0] == g["shadow"][0] == 320 * 240 and sum(g["traced"][1:]) == 0
    # the first frame and the one-shot (torch-free process) by phase
    fb = d["first_frame_breakdown"]
    assert {"scene_load_ms", "context_ms", "upload_ms", "first_render_ms", "d2h_ms"} <= set(fb)
    for k in ("one_shot", "one_shot_sdma_copy"):  # blit-kernel frame copy (the CLI's), runtime default (SDMA)
        os_ = d[k]
        assert os_["total_ms"] >= os_["render_ms"] > 0 and os_["context_ms"] > 0, (k, os_)
        assert os_["runs"] == 3 and len(os_["total_ms_samples"]) == 3  # median of three fresh processes
    # the strong-scaling series at every N (here N = 1): configs[3] and [4] split by the group context
    assert "NOT a scaling result" in d["scaling_note"]
    assert set(d["tile_split"]) == {"cover", "table"}
    for name, ts in d["tile_split"].items():
        assert ts["config"]["width"] == 3840 and ts["config"]["height"] == 2160 and ts["config"]["scene"] == name
        assert ts["scaling"] == "strong" and set(ts["gather_variants"]) == {"rccl", "peer"}
        for k in ("render_ms_per_shard", "single_gpu_ms_per_step", "speedup_vs_1gpu", "value"):
            assert ts[k] > 0, (name, k)


def test_dumped_frame_above_the_limit_is_a_fixed_choice_of_rows(tmp_path):
    """--dump-outputs: a u8 canvas becomes float32; above the size limit the
    same whole rows are kept in every run and listed in frame_rows.npy."""
    import numpy as np
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    frame = (np.arange(40 * 16 * 3) % 251).astype(np.uint8).reshape(40, 16, 3)
    kinds = {"primary": 640, "shadow": 1280, "reflect": 3, "refract": 2}
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), frame, kinds, limit=10 * 16 * 3 * 4 + 5)
    rows = np.load(tmp_path / "a" / "frame_rows.npy")
    got = np.load(tmp_path / "a" / "frame.npy")
    assert rows.dtype == np.float64 and len(rows) == 10 and len(set(rows)) == 10 and list(rows) == sorted(rows)
    assert got.dtype == np.float32 and np.array_equal(got, frame[rows.astype(int)].astype(np.float32))
    assert np.array_equal(rows, np.load(tmp_path / "b" / "frame_rows.npy"))
    assert list(np.load(tmp_path / "a" / "rays_by_kind.npy")) == [640, 1280, 3, 2]
    # a frame within the limit is written whole, f64 stays f64, and no stale row list is left
    bench.write_outputs(str(tmp_path / "a"), frame.astype(np.float64) / 255, kinds)
    whole = np.load(tmp_path / "a" / "frame.npy")
    assert whole.dtype == np.float64 and np.array_equal(whole, frame.astype(np.float64) / 255)
    assert not (tmp_path / "a" / "frame_rows.npy").exists()


FULL_ONLY = {"tile_split", "cpu_baseline", "one_shot", "one_shot_sdma_copy", "host_frame_ms", "rays_by_generation",
             "cold_kernel_ms", "device_state", "roofline", "frame_latency_ms"}


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_the_last_frame(gpu_ctx, rtc, tmp_path):
    """Without --full: the headline figures and nothing that takes a run of its
    own; --steps is the number of timed steps (7 is no multiple of the three
    frames in flight: the last frame lies in the first context's buffer), and
    --dump-outputs writes that frame, bit for bit what the library renders."""
    import numpy as np
    from conftest import scene_fixture
    d = _run("--gpus", "1", "--steps", "7", "--warmup", "2", "--warmup-ms", "0", "--width", "320", "--height", "240",
             "--dump-outputs", str(tmp_path / "out"))
    assert d["metric"] == "Mray/s (primary+secondary) and ms/frame at 1920x1080" and d["unit"] == "Mray/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["n_gpus"] == 1
    assert d["steps"] == 7 and d["warmup"] == 2 and d["frames_in_flight"] == 3
    assert d["ms_per_step"] > 0 and d["config"]["rays_per_frame"] == 2 * 320 * 240
    # value is the timed steps' rays over their time
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 2 * 320 * 240 / 1e6) < 1e-6 * d["value"]
    assert d["rays_by_kind"] == {"primary": 320 * 240, "shadow": 320 * 240, "reflect": 0, "refract": 0}
    assert not FULL_ONLY & set(d), sorted(FULL_ONLY & set(d))
    assert sorted(os.listdir(tmp_path / "out")) == ["frame.npy", "rays_by_kind.npy"]
    frame = np.load(tmp_path / "out" / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (240, 320, 3)
    assert list(np.load(tmp_path / "out" / "rays_by_kind.npy")) == [320 * 240, 320 * 240, 0, 0]
    scene = scene_fixture("three_sphere_scene")
    gpu_ctx.upload(scene)
    want, _ = gpu_ctx.render(rtc.camera_resize(scene.camera, 320, 240), 5, precision="f32")
    assert np.array_equal(frame, want)


@pytest.mark.gpu
def test_bench_tiled_line_on_one_gpu():
    """--mode tiled through librtc's RCCL group with one rank (the driver's
    N > 1 default, scaled down): per-shard render, gather and end-to-end
    milliseconds and the same workload on one GPU are reported."""
    d = _run("--full", "--mode", "tiled", "--steps", "10", "--warmup", "2", "--width", "640", "--height", "360",
             "--no-cpu-baseline")
    assert KEYS <= set(d)
    assert d["scaling"] == "strong" and d["config"]["mode"] == "tiled" and d["config"]["scene"] == "cover"
    assert d["config"]["out"] == "u8" and d["config"]["parallelism"] == "tilesx1"
    for k in ("render_ms_per_shard", "gather_ms", "frame_ms", "single_gpu_ms_per_step", "speedup_vs_1gpu"):
        assert d[k] > 0, k
    assert d["roofline"]["bound"] == "valu"
    # both ways of assembling the frame on rank 0, measured over the same steps
    gv = d["gather_variants"]
    assert set(gv) == {"rccl", "peer"} and d["gather"] == "rccl"
    for v in gv.values():
        assert v["ms_per_step"] > 0 and v["frame_ms"] > 0 and v["render_ms_per_shard"] > 0


@pytest.mark.gpu
def test_bench_pool_scene_reports_cold_launch():
    d = _run("--full", "--scene", "reflect_refract", "--steps", "10", "--warmup", "2", "--width", "320",
             "--height", "240", "--no-cpu-baseline")
    assert d["cold_kernel_ms"] > 0 and d["host_frame_ms"] > 0


@pytest.mark.gpu
def test_bench_two_ranks_frames_weak_scaling():
    """N > 1: one process per GPU (here two ranks rehearsed on the one GPU,
    BENCH_SHARE_GPU=1): each rank renders its own configs[1] frames, the line
    is the whole job's rays over the slowest rank's time, "scaling": "weak"."""
    env = dict(os.environ, BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29533", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--mode", "frames", "--steps", "10", "--warmup", "2", "--width", "320",
                        "--height", "240"], capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["parallelism"] == "framesx2"
    assert d["config"]["rays_per_frame"] == 2 * 320 * 240 and "tile_split" not in d
    # the job's rays: both ranks' frames
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 2 * 2 * 320 * 240 / 1e6) < 1e-6 * d["value"]
