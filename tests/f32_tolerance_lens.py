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
