"""The C++ YAML scene loader (csrc/scene_loader.cpp) against the semantics of
the reference's ray-tracer-cli/src/scene_loader.rs.

* parse_f64 / parse_array_of_3 known answers: scene_loader.rs:378-398;
* quirks of SceneParser: named transforms right-multiply
  while inline ops left-multiply (scene_loader.rs:200-233), `extend`
  (scene_loader.rs:106-112), `value:` indirection, `width`/`height` parsed
  as f64 and cast with `as u32` (scene_loader.rs:256-257), unknown `add:`
  kinds ignored (scene_loader.rs:330), cylinder/cone min/max/closed
  (scene_loader.rs:293-328), defaults (material.rs:157-161);
* the committed fixtures tests/golden/scenes/*.json are what the loader makes
  of the reference's scenes/*.yaml (kept as tests/golden/scenes_yaml/*.yaml).
  Those fixtures feed the oracle that reproduces the reference's PNGs
  bit-exactly (test_oracle_images.py), which pins this loader end to end.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, SCENES_YAML, scene_fixture

CAMERA = """
- add: camera
  width: 8
  height: 6
  field-of-view: 1.0
  from: [0, 0, -5]
  to: [0, 0, 0]
  up: [0, 1, 0]
"""


def load(rtc, body):
    return rtc.load_scene_text(CAMERA + body)


def inv_of(rtc, m):
    return rtc.matrix_inverse(np.asarray(m, dtype=np.float64)).reshape(16)


@pytest.mark.parametrize("text,expected", [("1", 1.0), ("1.0", 1.0), (".0", 0.0), ("0.", 0.0), ("0", 0.0)])
def test_parse_f64_known_answers(rtc, text, expected):
    """scene_loader.rs:378-388"""
    s = load(rtc, f"- add: light\n  at: [{text}, 2, 3]\n  intensity: [1, 1, 1]\n")
    assert s.lights[0].position[0] == expected and list(s.lights[0].position)[1:] == [2.0, 3.0]


@pytest.mark.parametrize("text,expected", [("[0.0, .0, 1.0]", [0.0, 0.0, 1.0]), ("[.0, 1.0, 1]", [0.0, 1.0, 1.0]),
                                           ("[10, 0, 1]", [10.0, 0.0, 1.0])])
def test_parse_array_of_3_known_answers(rtc, text, expected):
    """scene_loader.rs:390-398"""
    s = load(rtc, f"- add: light\n  at: {text}\n  intensity: [1, 1, 1]\n")
    assert list(s.lights[0].position) == expected


def test_named_transform_right_multiplies_inline_ops_left_multiply(rtc):
    from rtc_amd import world as W
    s = load(rtc, """
- define: grow-transform
  value:
    - [scale, 2, 2, 2]
- add: sphere
  transform:
    - [translate, 1, 0, 0]
    - grow-transform
    - [rotate-y, 0.5]
""")
    # T = rotate_y * ((translate * I) * grow)
    t = W.mat_mul(W.rotation_y(0.5), W.mat_mul(W.mat_mul(W.translation(1, 0, 0), np.eye(4)), W.scaling(2, 2, 2)))
    assert np.array_equal(np.array(s.shapes[0].inverse), inv_of(rtc, t))
    other = W.mat_mul(W.rotation_y(0.5), W.mat_mul(W.scaling(2, 2, 2), W.translation(1, 0, 0)))
    assert not np.allclose(np.array(s.shapes[0].inverse), inv_of(rtc, other))


def test_material_extend_value_and_defaults(rtc):
    s = load(rtc, """
- define: base-material
  value:
    color: [0.2, 0.3, 0.4]
    ambient: 0.5
- define: shiny-material
  extend: base-material
  value:
    diffuse: 0.3
    reflective: 0.25
- add: sphere
  material: shiny-material
- add: plane
""")
    shiny = s.materials[s.shapes[0].material]
    assert list(shiny.color) == [0.2, 0.3, 0.4] and shiny.ambient == 0.5 and shiny.diffuse == 0.3
    assert shiny.reflectiveness == 0.25
    default = s.materials[s.shapes[1].material]  # material.rs:157-161
    assert list(default.color) == [1.0, 1.0, 1.0]
    assert (default.ambient, default.diffuse, default.specular, default.shininess) == (0.1, 0.9, 0.9, 200.0)
    assert (default.reflectiveness, default.transparency, default.refractive_index) == (0.0, 0.0, 1.0)
    assert default.casts_shadow == 1 and default.pattern == -1
    assert list(s.shapes[1].inverse) == list(np.eye(4).reshape(16))


def test_camera_size_is_cast_like_as_u32(rtc):
    s = rtc.load_scene_text(CAMERA.replace("width: 8", "width: 10.7").replace("height: 6", "height: 6.2"))
    assert (s.camera.width, s.camera.height) == (10, 6)
    ref = rtc.camera_make(10, 6, 1.0, (0, 0, -5), (0, 0, 0), (0, 1, 0))
    assert bytes(s.camera) == bytes(ref)


def test_unknown_add_kinds_are_ignored_and_cylinder_fields_parse(rtc):
    s = load(rtc, """
- add: triangle
- add: group
- add: cylinder
  min: -1
  max: 2.5
  closed: true
- add: cone
""")
    assert len(s.shapes) == 2
    cyl, cone = s.shapes[0], s.shapes[1]
    assert (cyl.kind, cyl.minimum, cyl.maximum, cyl.closed) == (3, -1.0, 2.5, 1)
    assert (cone.kind, cone.closed) == (4, 0)
    assert cone.minimum == -np.finfo(np.float64).max and cone.maximum == np.finfo(np.float64).max


def test_casts_shadow_and_patterns(rtc):
    s = load(rtc, """
- add: plane
  material:
    casts-shadow: false
    pattern:
      type: checkers
      colors:
        - [1, 1, 1]
        - [0, 0, 0]
      transform:
        - [scale, 0.5, 0.5, 0.5]
""")
    m = s.materials[s.shapes[0].material]
    assert m.casts_shadow == 0 and m.pattern == 0
    p = s.patterns[0]
    assert p.kind == 3 and list(p.color_a) == [1.0, 1.0, 1.0] and list(p.color_b) == [0.0, 0.0, 0.0]
    assert np.allclose(np.array(p.inverse).reshape(4, 4), np.diag([2.0, 2.0, 2.0, 1.0]), rtol=0, atol=0)


@pytest.mark.parametrize("text", ["- add: light\n  at: [1, 2\n", "[unclosed", ""])
def test_malformed_yaml_is_an_error(rtc, text):
    with pytest.raises(rtc.RenderError):
        rtc.load_scene_text(text)


def test_missing_file_is_an_io_error(rtc):
    with pytest.raises(rtc.RenderError) as e:
        rtc.load_scene("/nonexistent/scene.yaml")
    assert e.value.code == -7  # RT_ERR_IO


FIXTURES = sorted(f[:-5] for f in os.listdir(os.path.join(GOLDEN, "scenes")) if f.endswith(".json"))


@pytest.mark.parametrize("name", FIXTURES)
def test_loader_reproduces_committed_fixtures(rtc, name):
    got = rtc.load_scene(os.path.join(SCENES_YAML, f"{name}.yaml"))
    want = scene_fixture(name)
    for field in ("shapes", "materials", "patterns", "lights"):
        a, b = getattr(got, field), getattr(want, field)
        assert len(a) == len(b) and bytes(a) == bytes(b), f"{name}: {field} differ"
    assert bytes(got.camera) == bytes(want.camera)


def test_yaml_camera_matches_camera_new(rtc):
    """Camera::new + set_transformation (camera.rs:25-49, 114-127) through both paths."""
    s = rtc.load_scene_text(CAMERA)
    c = rtc.camera_make(8, 6, 1.0, (0, 0, -5), (0, 0, 0), (0, 1, 0))
    half_view = math.tan(0.5)
    assert c.half_width == half_view and c.half_height == half_view / (8 / 6)
    assert c.pixel_size == (half_view * 2.0) / 8.0
    assert bytes(s.camera) == bytes(c)
    assert C.sizeof(s.camera) == C.sizeof(c)
