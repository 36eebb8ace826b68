"""The `rtc` CLI's lens flags: --aperture R --focus D [--lens-jitter[=SEED]] (rt_render_lens)."""
import subprocess

import numpy as np
import pytest

from test_cli import CLI, SCENE, read_ppm


def _run(*args):
    return subprocess.run([CLI, "a.yaml", "b.ppm", *args], capture_output=True, text=True)


def test_usage_names_the_lens_flags():
    r = subprocess.run([CLI], capture_output=True, text=True)
    assert r.returncode != 0 and "--aperture R --focus D [--lens-jitter[=SEED]]" in r.stderr


def test_parse_errors_have_their_own_texts():
    for bad in ("-0.1", "wide", "1x", "nan", "inf"):
        r = _run("--aperture", bad, "--focus", "5")
        assert r.returncode == 2 and "--aperture takes a lens radius" in r.stderr, (bad, r.stderr)
    for bad in ("0", "-2", "far", "5m", "nan", "inf"):
        r = _run("--aperture", "0.1", "--focus", bad)
        assert r.returncode == 2 and "--focus takes a focal distance" in r.stderr, (bad, r.stderr)
    for bad in ("--lens-jitter=", "--lens-jitter=x", "--lens-jitter=-1", "--lens-jitter=4294967296"):
        r = _run("--aperture", "0.1", "--focus", "5", bad)
        assert r.returncode == 2 and "--lens-jitter takes an optional =SEED" in r.stderr, (bad, r.stderr)
    for missing in (("--aperture",), ("--aperture", "0.1", "--focus")):
        assert _run(*missing).returncode == 2
    r = _run("--aperture", "0.1")
    assert r.returncode == 2 and "--aperture needs --focus D" in r.stderr
    r = _run("--aperture", "0.1", "--samples", "2", "--lens-jitter=3")
    assert r.returncode == 2 and "--aperture needs --focus D" in r.stderr
    for alone in (("--focus", "5"), ("--lens-jitter",)):
        r = _run(*alone)
        assert r.returncode == 2 and "give --aperture R" in r.stderr, (alone, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("jitter", [(), ("--lens-jitter=9",)])
def test_cli_render_equals_render_lens(tmp_path, rtc, gpu_ctx, jitter):
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    out = tmp_path / "out.ppm"
    r = subprocess.run([CLI, str(yaml), str(out), "--width", "70", "--height", "22", "--samples", "2", "--aperture", "0.2",
                        "--focus", "5.5", *jitter, "--ppm-binary", "-q"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    scene = rtc.load_scene(str(yaml))
    gpu_ctx.upload(scene)
    want, _ = gpu_ctx.render_lens(rtc.camera_resize(scene.camera, 70, 22), 2, rtc.Lens(0.2, 5.5, bool(jitter), 9 if jitter else 0),
                                  6, precision="f32", out_format="u8")
    assert np.array_equal(read_ppm(out, b"P6"), want)
    pin, _ = gpu_ctx.render_supersampled(rtc.camera_resize(scene.camera, 70, 22), 2, 6, precision="f32", out_format="u8")
    assert not np.array_equal(want, pin)
