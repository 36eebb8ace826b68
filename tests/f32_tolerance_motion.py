"""f32 motion (rt_trace_rays_timed, rt_render_shutter) against the f64 oracle in the world at
each ray's time (tests/motion_reference.py): the timed batches of tests/motion_worlds.py (2048 rays) and the
70 x 22, n = 2 shutter frames over [0, 1] at the cell centres, pinhole and lens.

The observed share of rays (batches) and pixels (frames) within 2/255 after quantization, measured on MI355X
against the oracle (never against the f32 kernels themselves) and recorded in profiles/motion_parity.json; the
test's floor is the share minus 0.005, the project's rule.  Keys: ("batch", world) and
("frame", world, with a lens).
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
}
