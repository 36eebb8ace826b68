"""The inputs of the random motion tests (tests/test_gpu_motion_random.py, tests/test_gpu_motion_meshes.py),
checked without a GPU: on the oracle and the numpy references alone.

  - random_world() is byte-stable: the tables of seeds 0 to 47 hash to what they hashed to before the function
    moved out of tests/test_gpu_random_worlds.py (tests/golden/random_worlds_sha256.json);
  - the conditions that make the GPU tests of the random moving worlds say something.  None of them is a
    tolerance: they are conditions on the draw (tests/random_moving_worlds.py), and a seed that missed one would
    call for another draw, not another condition;
  - no ray of motion_worlds.maps()'s batch and frames lands within 1e-6 of a plane where its image patterns and
    the oracle's stripes differ;
  - the numpy references of the moving smooth and textured triangles leave out at most 1 % of the rays of each
    world of tests/motion_mesh_worlds.py (rays whose decision margin is at most 1e-9).
"""
import json
import os

import numpy as np
import pytest

import motion_mesh_worlds as MM
import motion_reference as MR
import motion_worlds as MW
import random_moving_worlds as RM
import random_worlds

HERE = os.path.dirname(os.path.abspath(__file__))


def test_random_world_is_byte_stable_across_its_move():
    with open(os.path.join(HERE, "golden", "random_worlds_sha256.json")) as f:
        want = json.load(f)["sha256"]
    assert sorted(want, key=int) == [str(s) for s in range(48)]
    for seed in range(48):
        assert random_worlds.tables_sha256(*random_worlds.random_world(seed)) == want[str(seed)], seed


def test_the_base_world_of_a_moving_seed_is_the_static_seeds_world():
    """(the motion list has a generator of its own; the area light of every third seed replaces its first light)"""
    for seed in RM.SEEDS:
        moving, cam, depth = RM.world(seed)
        base, bcam, bdepth = random_worlds.random_world(seed)
        assert bytes(moving.shapes) == bytes(base.shapes) and bytes(moving.materials) == bytes(base.materials)
        assert bytes(moving.patterns) == bytes(base.patterns) and bytes(cam) == bytes(bcam) and depth == bdepth
        if seed % 3:
            assert bytes(moving.lights) == bytes(base.lights) and not moving.lit
        else:
            lights = moving.expanded_lights()
            assert len(lights) == len(base.lights) + 3 and len(moving.area_lights) == 1
            cells = lights[len(base.lights) - 1:]
            assert np.allclose(np.mean([c.position[:] for c in cells], axis=0), base.lights[0].position[:], atol=1e-12)
            assert np.allclose(np.sum([c.intensity[:] for c in cells], axis=0), base.lights[0].intensity[:], atol=1e-15)
            assert sorted({abs(c.position[0] - base.lights[0].position[0]) for c in cells}) == [0.25]


def test_the_upload_accepts_every_motion_list(rtc):
    """rt_scene_upload_moving with a null context: the lists pass their checks and the context is looked at last."""
    for seed in RM.SEEDS:
        tables = RM.world(seed)[0]
        assert rtc._lib.rt_scene_upload_moving(None, *tables.moving_args()) != 0
        assert rtc._lib.rt_last_error().decode() == "null context", seed
        v = RM.velocities(tables)
        assert len(v) == len(tables.motion) and all(np.abs(q).max() <= 2.0 and np.abs(q).max() > 0.0 for q in v.values())
        assert not tables.at_time(0.3).moving


def test_value_equal_shapes_move_together():
    for seed in RM.SEEDS:
        tables = RM.world(seed)[0]
        v, cls = RM.velocities(tables), RM.classes(tables)
        for i, c in enumerate(cls):
            assert (i in v) == (c in v) and (i not in v or np.array_equal(v[i], v[c])), (seed, i)
        # ... so the world at every time has the classes of the moving world
        for tau in RM.TIMES:
            assert RM.classes(tables.at_time(tau)) == cls


def test_every_kind_moves_and_the_hard_cases_are_there():
    moved = {k: 0 for k in RM.KINDS.values()}
    pairs = glass = 0
    for seed in RM.SEEDS:
        tables, _, depth = RM.world(seed)
        v, cls = RM.velocities(tables), RM.classes(tables)
        kinds = {RM.KINDS[tables.shapes[i].kind] for i in v}
        assert kinds - {"plane"}, seed  # a bounded shape moves in every world
        for k in kinds:
            moved[k] += 1
        pairs += any(c != i and i in v for i, c in enumerate(cls))
        glass += depth >= 2 and any(tables.materials[tables.shapes[i].material].transparency > 0 for i in v)
    print(moved, "worlds with a moving pair:", pairs, "with a moving transparent shape at depth >= 2:", glass)
    assert all(n >= 2 for n in moved.values()), moved
    assert pairs >= 2 and glass >= 4


def test_batch_origins_lie_inside_movers():
    worlds = 0
    for seed in RM.SEEDS:
        tables = RM.world(seed)[0]
        rays, times = RM.batch(seed)
        assert rays.shape == (RM.N_RAYS, 6) and np.allclose(np.linalg.norm(rays[:, 3:], axis=1), 1.0, atol=1e-12)
        assert all(np.array_equal(times[k::4], np.full(RM.N_RAYS // 4, RM.TIMES[k])) for k in range(4))
        found = 0
        for tau in RM.TIMES:
            at = tables.at_time(tau)
            for i in RM.velocities(tables):
                found += int(RM.inside(at, i, rays[times == tau, :3]).sum())
        worlds += found > 0
    print("worlds with a batch origin inside a mover at its ray's time:", worlds)
    assert worlds >= 3


@pytest.mark.parametrize("seed", RM.SEEDS)
def test_the_random_batches_see_the_motion(oracle, seed):
    """tests/test_gpu_motion.py's bar: at least 5 % of the rays differ by more than 1e-6 from the world at tau = 0."""
    cols, _ = RM.batch_reference(oracle, seed)
    assert np.isfinite(cols).all()
    share = float((np.abs(cols - RM.static_reference(oracle, seed)).max(axis=1) > 1e-6).mean())
    print(f"seed {seed}: {share:.3f} of the rays see the motion")
    assert share >= 0.05, (seed, share)


def test_no_ray_of_the_maps_world_lands_within_1e_6_of_the_planes(oracle, rtc):
    """The oracle's stripes moved by +-1e-6 along x give the same batch and the same 70 x 22 frames (pinhole and
    lens), to the bit: no hit lies within 1e-6 of a plane where the image patterns of motion_worlds.maps() and
    the stripes differ (tests/test_uv_maps_cpu.py's probe, at each ray's time)."""
    rays, times = MW.batch("maps")
    got = []
    for shift in (0.0, 1e-6, -1e-6):
        scene = MW.maps(mapped=False, shift=shift)[0]
        out = [MR.trace(oracle, scene, rays, times, 2)[0]]
        out += [MR.frame(oracle, scene, MW.camera(), rtc, 70, 22, 2, (0.0, 1.0, False, 0), 2, lens)[0]
                for lens in (None, (0.05, 5.0, False, 0))]
        got.append(out)
    for other in got[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got[0], other))
    # (the probe is not blind: a shift of a tenth of a stripe changes all three)
    far = MW.maps(mapped=False, shift=0.1)[0]
    assert not np.array_equal(MR.trace(oracle, far, rays, times, 2)[0], got[0][0])


@pytest.mark.parametrize("name", MM.NAMES)
def test_the_mesh_references_leave_out_at_most_one_percent(name):
    """The restatement alone, in the world at each ray's time: at most 1 % of the batch's rays sit within 1e-9 of
    a decision fence (a triangle's edge, the nearest filter's texel change, a wrap point) and are left out of the
    GPU comparison; a good share of the others hit a mover, at every time."""
    rays, times = MM.batch(name)
    cols, hit, margin, kept = MM.reference(name)
    assert rays.shape == (48 * 36 + 512, 6) and np.isfinite(cols).all()
    left_out = float((~kept).mean())
    on_mover = np.isin(hit["shape"], MM.mover_shapes(name)) & kept
    print(f"{name}: {left_out:.4f} left out, {on_mover.mean():.3f} of the rays hit a mover, smallest margin kept {margin[kept].min():.3g}")
    assert left_out <= MM.MAX_LEFT_OUT, (name, left_out)
    assert all(on_mover[times == tau].mean() >= 0.1 for tau in MM.TIMES), name
