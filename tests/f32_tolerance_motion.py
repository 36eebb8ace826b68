"""f32 motion (rt_trace_rays_timed, rt_render_shutter) against the f64 oracle in the world at
each ray's time (tests/motion_reference.py): the timed batches of tests/motion_worlds.py (2048 rays) and the
70 x 22, n = 2 shutter frames over [0, 1] at the cell centres, pinhole and lens.

The observed share of rays (batches) and pixels (frames) within 2/255 after quantization, measured on MI355X
against the oracle (never against the f32 kernels themselves) and recorded in profiles/motion_parity.json; the
test's floor is the share minus 0.005, the project's rule.  Keys: ("batch", world) and
("frame", world, with a lens).

The seeded random moving worlds (tests/random_moving_worlds.py, tests/test_gpu_motion_random.py): ("random_batch",
seed), the 2048 rays of the seed's batch, and ("random_frame", seed), its 70 x 22, n = 2 shutter frame, both against
the oracle, floor the share minus 0.005.  LIKE_OBSERVED is the share of each seed's f32 timed batch within 2/255
of the f32 static batch of an upload of at_time(tau): two f32 kernels that differ only in how the displacement is
rounded.  Its floor LIKE_FLOOR is one value for all seeds, the smallest observed share minus 0.002.

The moving smooth and textured triangles (tests/motion_mesh_worlds.py, tests/test_gpu_motion_meshes.py) have no
oracle world: ("mesh_batch", world) is the share of the f32 timed batch within 2/255 of the f64 device batch, which
the f64 tests hold to 1e-9 of the numpy restatements; floor the share minus 0.005.  STATIC_TWINS names, for each,
the static world of profiles/smooth_parity.json or profiles/texture_parity.json nearest to it with its recorded
share of rays, for comparison: no moving share is below its twin's.
"""
SHARE_OBSERVED = {
    ("batch", "far_sphere"): 1.0,
    ("batch", "far_cube"): 1.0,
    ("batch", "far_cylinder"): 1.0,
    ("batch", "far_triangle"): 1.0,
    ("batch", "far_instance"): 1.0,
    ("batch", "shadow"): 1.0,
    ("batch", "plane"): 1.0,
    ("batch", "glass"): 0.999023,
    ("batch", "glass_single"): 0.998535,
    ("batch", "pattern"): 1.0,
    ("batch", "area"): 1.0,
    ("batch", "tree"): 1.0,
    ("frame", "far_sphere", False): 0.968831,
    ("frame", "far_sphere", True): 0.995455,
    ("frame", "far_cube", False): 0.97013,
    ("frame", "far_cube", True): 0.995455,
    ("frame", "far_cylinder", False): 0.969481,
    ("frame", "far_cylinder", True): 0.995455,
    ("frame", "far_triangle", False): 0.968831,
    ("frame", "far_triangle", True): 0.995455,
    ("frame", "far_instance", False): 0.966883,
    ("frame", "far_instance", True): 0.995455,
    ("frame", "shadow", False): 0.95974,
    ("frame", "shadow", True): 0.994156,
    ("frame", "plane", False): 0.98961,
    ("frame", "plane", True): 0.997403,
    ("frame", "glass", False): 0.970779,
    ("frame", "glass", True): 0.996753,
    ("frame", "glass_single", False): 0.970779,
    ("frame", "glass_single", True): 0.996753,
    ("frame", "pattern", False): 0.968831,
    ("frame", "pattern", True): 0.996753,
    ("frame", "area", False): 0.966234,
    ("frame", "area", True): 0.994805,
    ("frame", "tree", False): 1.0,
    ("frame", "tree", True): 1.0,
    ("batch", "maps"): 1.0,
    ("frame", "maps", False): 0.972727,
    ("frame", "maps", True): 0.995455,
    ("random_batch", 0): 0.999512,
    ("random_batch", 1): 1.0,
    ("random_batch", 2): 1.0,
    ("random_batch", 3): 1.0,
    ("random_batch", 4): 1.0,
    ("random_batch", 5): 1.0,
    ("random_batch", 6): 1.0,
    ("random_batch", 7): 1.0,
    ("random_batch", 8): 1.0,
    ("random_batch", 9): 1.0,
    ("random_batch", 10): 1.0,
    ("random_batch", 11): 1.0,
    ("random_batch", 12): 1.0,
    ("random_batch", 13): 1.0,
    ("random_batch", 14): 1.0,
    ("random_batch", 15): 1.0,
    ("random_batch", 16): 1.0,
    ("random_batch", 17): 1.0,
    ("random_batch", 18): 0.996582,
    ("random_batch", 19): 1.0,
    ("random_batch", 20): 1.0,
    ("random_batch", 21): 1.0,
    ("random_batch", 22): 1.0,
    ("random_batch", 23): 1.0,
    ("random_frame", 0): 0.999351,
    ("random_frame", 1): 1.0,
    ("random_frame", 2): 0.999351,
    ("random_frame", 3): 0.998052,
    ("random_frame", 4): 1.0,
    ("random_frame", 5): 0.998701,
    ("random_frame", 6): 0.999351,
    ("random_frame", 7): 1.0,
    ("random_frame", 8): 1.0,
    ("random_frame", 9): 1.0,
    ("random_frame", 10): 1.0,
    ("random_frame", 11): 1.0,
    ("random_frame", 12): 1.0,
    ("random_frame", 13): 0.999351,
    ("random_frame", 14): 0.999351,
    ("random_frame", 15): 1.0,
    ("random_frame", 16): 1.0,
    ("random_frame", 17): 0.999351,
    ("random_frame", 18): 0.985714,
    ("random_frame", 19): 1.0,
    ("random_frame", 20): 1.0,
    ("random_frame", 21): 0.998701,
    ("random_frame", 22): 1.0,
    ("random_frame", 23): 1.0,
    ("mesh_batch", "smooth_instance"): 1.0,
    ("mesh_batch", "flat_instance"): 1.0,
    ("mesh_batch", "smooth_tree"): 1.0,
    ("mesh_batch", "texture_nearest_flat"): 1.0,
    ("mesh_batch", "texture_nearest_smooth"): 1.0,
    ("mesh_batch", "texture_bilinear_flat"): 1.0,
    ("mesh_batch", "texture_bilinear_smooth"): 1.0,
    ("mesh_batch", "texture_instance"): 1.0,
}

LIKE_OBSERVED = {seed: 1.0 for seed in range(24)}  # every seed: all 2048 rays within 2/255
LIKE_OBSERVED_MIN = min(LIKE_OBSERVED.values())    # 1.0
LIKE_FLOOR = 0.998                                 # the smallest observed share, 1.0, less 0.002

STATIC_TWINS = {
    "smooth_instance": ("smooth_parity.json ico alone", 1.0),
    "flat_instance": ("smooth_parity.json ico alone", 1.0),
    "smooth_tree": ("smooth_parity.json ico alone", 1.0),
    "texture_nearest_flat": ("texture_parity.json ico nearest", 0.999755859375),
    "texture_nearest_smooth": ("texture_parity.json ico nearest", 0.999755859375),
    "texture_bilinear_flat": ("texture_parity.json ico bilinear", 0.999755859375),
    "texture_bilinear_smooth": ("texture_parity.json ico bilinear", 0.999755859375),
    "texture_instance": ("texture_parity.json tori", 0.99951171875),
}
