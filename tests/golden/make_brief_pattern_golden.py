"""Writes tests/golden/brief_pattern.npz: the four 256-entry test-pair lists of a BRIEF pattern file (the reference's
config/brief_pattern.yml, settings only) as int8 arrays x1, y1, x2, y2, read through keyframe.load_brief_pattern.

    python tests/golden/make_brief_pattern_golden.py PATH/brief_pattern.yml
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import isvins_loader  # noqa: E402

isvins_loader.load()
from isvins_amd import keyframe  # noqa: E402

if __name__ == "__main__":
    pat = keyframe.load_brief_pattern(sys.argv[1])
    np.savez(os.path.join(HERE, "brief_pattern.npz"), **{k: pat[k] for k in ("x1", "y1", "x2", "y2")})
    print({k: (v.dtype, v.shape, int(v.min()), int(v.max())) for k, v in pat.items()})
