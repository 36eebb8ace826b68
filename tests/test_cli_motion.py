"""The `rtc` CLI's motion flags: --move I:vx,vy,vz, --instance FILE:tx,ty,tz[:s][:v=vx,vy,vz] and
--shutter open,close[:jitter=SEED] (rt_scene_upload_moving, rt_render_shutter)."""
import subprocess

import numpy as np
import pytest

import motion_worlds as MW
from test_cli import CLI, SCENE, read_ppm


def _run(*args):
    return subprocess.run([CLI, "a.yaml", "b.ppm", *args], capture_output=True, text=True)


def test_usage_names_the_motion_flags():
    r = subprocess.run([CLI], capture_output=True, text=True)
    assert r.returncode != 0
    assert "[--move I:vx,vy,vz]... [--shutter open,close[:jitter=SEED]]" in r.stderr
    assert "[--instance MESH.obj:tx,ty,tz[:s][:v=vx,vy,vz]]..." in r.stderr


def test_parse_errors_have_their_own_texts():
    for bad in ("1", ":1,0,0", "x:1,0,0", "-1:1,0,0", "1:1,0", "1:1,0,0,0", "1:nan,0,0", "1:inf,0,0", "1.5:1,0,0", "1:a,b,c"):
        r = _run("--move", bad, "--shutter", "0,1")
        assert r.returncode == 2 and "--move takes I:vx,vy,vz" in r.stderr, (bad, r.stderr)
    r = _run("--move", "1:1,0,0", "--move", "1:0,2,0", "--shutter", "0,1")
    assert r.returncode == 2 and "--move names shape 1 twice" in r.stderr
    for bad in ("1", "0,", "a,b", "0,1,2", "1,0", "nan,1", "0,inf", "0,1:", "0,1:jitter", "0,1:jitter=", "0,1:jitter=x",
                "0,1:jitter=-1", "0,1:jitter=4294967296", "0,1:seed=3"):
        r = _run("--shutter", bad)
        assert r.returncode == 2 and "--shutter takes open,close[:jitter=SEED]" in r.stderr, (bad, r.stderr)
    for bad in ("m.obj:0,0,0:v=1,0", "m.obj:0,0,0:v=", "m.obj:0,0,0:2:v=nan,0,0", "m.obj:v=1,0,0", "m.obj:0,0,0:v=1,0,0,0"):
        r = _run("--instance", bad, "--shutter", "0,1")
        assert r.returncode == 2 and "--instance takes FILE:tx,ty,tz[:s][:v=vx,vy,vz]" in r.stderr, (bad, r.stderr)
    for missing in (("--move",), ("--shutter",)):
        assert _run(*missing).returncode == 2
    for movers in (("--move", "1:1,0,0"), ("--instance", "m.obj:0,0,0:v=1,0,0"), ("--instance", "m.obj:0,0,0:2:v=1,0,0")):
        r = _run(*movers)
        assert r.returncode == 2 and "describe motion: give --shutter open,close" in r.stderr, (movers, r.stderr)


def test_a_shape_beyond_the_scene_is_refused(tmp_path):
    yaml = tmp_path / "scene.yaml"
    yaml.write_text(SCENE)
    r = subprocess.run([CLI, str(yaml), str(tmp_path / "out.ppm"), "--move", "3:1,0,0", "--shutter", "0,1", "-q"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--move names shape 3, the scene has 3 shapes" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("jitter", [(), (":jitter=9",)])
@pytest.mark.parametrize("lens", [(), ("--aperture", "0.2", "--focus", "5.5")])
def test_cli_render_equals_render_shutter(tmp_path, rtc, gpu_ctx, jitter, lens):
    """The scene's sphere (shape 1) and an instanced octahedron move; the frame is Context.render_shutter's."""
    from rtc_amd import world as W
    yaml, obj, out = tmp_path / "scene.yaml", tmp_path / "octa.obj", tmp_path / "out.ppm"
    yaml.write_text(SCENE)
    obj.write_text(MW.OCTAHEDRON)
    r = subprocess.run([CLI, str(yaml), str(out), "--width", "70", "--height", "22", "--samples", "2", "--move", "1:1.5,0,0.25",
                        "--instance", f"{obj}:0.5,1.5,1:0.5:v=-2,0.5,0", "--shutter", "0.25,1" + "".join(jitter), *lens,
                        "--ppm-binary", "-q"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    scene = rtc.load_scene(str(yaml))
    # the CLI's world: the scene's tables, one default material more, the mesh placed by translation * scaling
    mats = (rtc.MaterialDesc * (len(scene.materials) + 1))(*scene.materials)
    m = mats[len(scene.materials)]
    m.color[:] = [1.0, 1.0, 1.0]
    m.ambient, m.diffuse, m.specular, m.shininess, m.refractive_index, m.casts_shadow, m.pattern = 0.1, 0.9, 0.9, 200.0, 1.0, 1, -1
    inst = (rtc.InstanceDesc * 1)()
    inst[0].mesh, inst[0].material = 0, len(scene.materials)
    inst[0].inverse[:] = [v for row in W.inverse(W.mat_mul(W.translation(0.5, 1.5, 1.0), W.scaling(0.5, 0.5, 0.5))) for v in row]
    motion = (rtc.MotionDesc * 2)()
    motion[0].target, motion[0].index = rtc.RT_MOVE_SHAPE, 1
    motion[0].velocity[:] = [1.5, 0.0, 0.25]
    motion[1].target, motion[1].index = rtc.RT_MOVE_INSTANCE, 0
    motion[1].velocity[:] = [-2.0, 0.5, 0.0]
    world = rtc.SceneTables(scene.shapes, mats, scene.patterns, scene.lights, scene.camera,
                            meshes=[MW.octahedron().shape_descs()], instances=inst, motion=motion)
    gpu_ctx.upload(world)
    assert gpu_ctx.motion_info()["moving_shapes"] == 1 and gpu_ctx.motion_info()["moving_instances"] == 1
    cam = rtc.camera_resize(scene.camera, 70, 22)
    want, _ = gpu_ctx.render_shutter(cam, 2, rtc.Shutter(0.25, 1.0, bool(jitter), 9 if jitter else 0),
                                     rtc.Lens(0.2, 5.5) if lens else None, 6, precision="f32", out_format="u8")
    assert np.array_equal(read_ppm(out, b"P6"), want)
    still, _ = gpu_ctx.render_supersampled(cam, 2, 6, precision="f32", out_format="u8")
    assert not np.array_equal(want, still)
