"""f32 lens frames (rt_render_lens) against the f64 oracle's mean over the lens rays of
tests/lens_reference.py: 320 x 200, n = 2, aperture 0.25, the focal distances of tests/test_gpu_lens.py.

The observed share of pixels within 2/255 after quantization, measured on MI355X against the oracle (never
against the f32 kernels themselves) and recorded in profiles/lens_parity.json; the test's floor is the share
minus 0.005, the project's rule.  Keys: (scene, hashed jitter).
"""
SHARE_OBSERVED = {
    ("three_sphere_scene", False): 1.0,
    ("three_sphere_scene", True): 1.0,
    ("shadow_puppets", False): 1.0,
    ("shadow_puppets", True): 0.999984375,
    ("reflect_refract", False): 0.999984375,
    ("reflect_refract", True): 0.999984375,
    ("refraction", False): 0.992640625,
    ("refraction", True): 0.99196875,
}

# Lens frames of the instanced and the textured build (tests/test_gpu_lens_builds.py): 160 x 100, n = 2, the
# lenses of tests/test_lens_builds_cpu.py, against the oracle's mean in the expansion's world (instanced) or the
# numpy references' (smooth, textured); recorded in profiles/lens_builds_parity.json.  Keys: (world, hashed
# jitter).  The smallest, 0.99975, is 0.00005 below the 0.9998 of the pinhole frames of tests/test_gpu_smooth.py
# and tests/test_gpu_texture.py: 4 pixels of 16000 on silhouettes of glass.
SHARE_OBSERVED.update({
    ("instanced three_tori", False): 1.0,
    ("instanced three_tori", True): 0.9998125,
    ("instanced nested_glass", False): 0.9999375,
    ("instanced nested_glass", True): 0.99975,
    ("smooth direct", False): 1.0,
    ("smooth direct", True): 1.0,
    ("smooth pool", False): 1.0,
    ("smooth pool", True): 1.0,
    ("textured direct", False): 1.0,
    ("textured direct", True): 1.0,
    ("textured pool", False): 1.0,
    ("textured pool", True): 1.0,
})
