"""Record tests/golden/refpin.npz from the compiled reference (oracle/_ref/libref_stvo.so, built by
`make -C oracle` where the reference tree is present): the inputs and the reference's own outputs of
tests/refpin_cases.py. The stereo window's four half-widths are read from the reference's text, the
assignment in src2/stereoFrame.cpp and the default of matching_s_ws in src2/config.cpp, not from include/plba.h.
Usage: python tools/make_refpin_golden.py
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pl-slam-plucker_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import ref_stereo as RS  # noqa: E402
import refpin_api as api  # noqa: E402
import refpin_cases as cases  # noqa: E402


def stereo_window():
    """(left, right, up, down) of the GridWindow that matchStereoPoints and matchStereoLines build."""
    text = open(os.path.join(api.REFERENCE, "src2", "stereoFrame.cpp")).read()
    found = re.findall(r"w\.width\s*=\s*std::make_pair\(\s*Config::matchingSWs\(\)\s*,\s*(\d+)\s*\);\s*"
                       r"w\.height\s*=\s*std::make_pair\(\s*(\d+)\s*,\s*(\d+)\s*\);", text)
    assert len(found) == 2 and found[0] == found[1], found      # the point and the line matcher, alike
    ws = re.findall(r"\bmatching_s_ws\s*=\s*(\d+)\s*;", open(os.path.join(api.REFERENCE, "src2", "config.cpp")).read())
    assert len(ws) == 1, ws
    right, up, down = (int(v) for v in found[0])
    return (int(ws[0]), right, up, down)


def main():
    assert api.available() and api.tree_present(), "build oracle/_ref/libref_stvo.so first: make -C oracle"
    w = stereo_window()
    out = cases.compute(api, w)
    # the open-gate frame must lose no match to a NaN, or the device test could not see every row
    f = cases.stereo_frame()
    got = RS.associate(f, RS.params(**cases.SC.CAMERA, matching_s_ws=w[0], **cases.OPEN_GATES))
    assert got["pt_src"].tolist() == np.flatnonzero(out["mg_stereo_pts_lr1"][:-1] >= 0).tolist()
    assert got["ls_src"].tolist() == np.flatnonzero(out["mg_stereo_lns_lr1"][:-1] >= 0).tolist()
    path = cases.GOLDEN
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays, stereo window", w)


if __name__ == "__main__":
    main()
