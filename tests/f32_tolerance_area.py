"""The f32 path's tolerance for worlds with area lights (tests/test_gpu_area_lights.py), beside
tests/f32_tolerance.py: the share of 64 x 32 frame pixels within 2/255 of the f64 device frame of the same
upload.  The yardstick is the share the light list's expansion reaches on the same world (its f32 frame
against its f64 frame, uploaded through the older entry points), less MARGIN: one pixel of the frame, since
shadow-edge decisions flip alike in both.  Observed on MI355X (profiles/area_light_parity.json,
scripts/area_light_parity.py): see FLOORS' comments.
"""
MARGIN = 0.0005  # one pixel of a 64 x 32 frame (1 / 2048 = 0.00049)
# world -> the recorded share of the expansion less MARGIN; (area upload, expansion) observed in the comments
FLOORS = {
    "opaque": 0.9995,  # (1.0, 1.0): 2048 and 2048 of 2048 pixels
    "mirror": 0.9995,  # (1.0, 1.0)
}
