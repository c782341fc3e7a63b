#!/usr/bin/env python3
"""Golden g30_motion_video: outputs of the reference's own pure-numpy ``resize_or_crop`` and ``crop_bottom``
(lib/utils/motion_video.py:6-38), captured by loading that file (read-only) with a stub ``cv2`` module -- run in the build container only:

    python tests/golden/gen_golden_video.py

Small random uint8 images (tens of pixels), one case per branch the reference can execute: wider / equal / narrower against taller /
equal / shorter, except narrower with another height (a numpy shape error there), with odd and even size differences (the centre crop and
the centring floor-divide).  Arrays only: inputs, the (width, height) / crop_length arguments and the reference's outputs.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import REF, save  # noqa: E402

# (h, w) of the input, (width, height) asked for
RESIZE_CASES = [((40, 37), (24, 30)),      # wider, taller: centre columns (odd difference), bottom rows
                ((21, 36), (24, 30)),      # wider, shorter: centre columns (even difference), bottom-aligned over white
                ((30, 29), (24, 30)),      # wider, same height
                ((30, 15), (24, 30)),      # narrower (odd difference), same height: centred over white
                ((30, 20), (24, 30)),      # narrower (even difference), same height
                ((47, 24), (24, 30)),      # same width, taller
                ((11, 24), (24, 30)),      # same width, shorter
                ((30, 24), (24, 30))]      # same size: returned as is
CROP_CASES = [((25, 19), 0), ((25, 19), 7), ((32, 16), 20), ((9, 5), 8)]


def main():
    sys.modules["cv2"] = types.ModuleType("cv2")
    spec = importlib.util.spec_from_file_location("ref_motion_video", os.path.join(REF, "lib", "utils", "motion_video.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rs = np.random.RandomState(30)
    out = {}
    for k, ((h, w), (width, height)) in enumerate(RESIZE_CASES):
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        out[f"resize/{k}/in"] = img
        out[f"resize/{k}/wh"] = np.array([width, height], np.int64)
        out[f"resize/{k}/out"] = np.asarray(ref.resize_or_crop(img.copy(), width, height)).astype(np.uint8)
    for k, ((h, w), n) in enumerate(CROP_CASES):
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        out[f"crop/{k}/in"] = img
        out[f"crop/{k}/n"] = np.array(n, np.int64)
        out[f"crop/{k}/out"] = np.asarray(ref.crop_bottom(img.copy(), n)).astype(np.uint8)
    save("g30_motion_video", **out)


if __name__ == "__main__":
    main()
