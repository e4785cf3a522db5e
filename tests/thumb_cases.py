"""The insets the map tests share (tests/test_thumb_host.py on the CPU, tests/test_gpu_map_insets.py on the device), on the
pictures of tests/map_cases.py."""
import numpy as np

PICTURES = [(64, 1), (64, 2), (160, 1), (160, 2)]      # width, views


def inset_cases(width, height):
    """name -> insets of a width x height picture: flush in each corner, two overlapping in both orders, a label partly
    outside the picture, no label"""
    rng = np.random.default_rng(width)
    a, b = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8), rng.integers(0, 256, (11, 7, 3), dtype=np.uint8)
    corners = [dict(index=0, at=(0, 0), label=(1, 1, "UAS7"), pixels=a), dict(index=1, at=(width - 7, 0), label=(width - 9, 3, "K2"), pixels=b),
               dict(index=0, at=(0, height - 9), label=(2, height - 5, "cam (a)"), pixels=a),
               dict(index=1, at=(width - 7, height - 11), label=(width - 20, height - 12, "X,Y"), pixels=b)]
    over = [dict(index=2, at=(20, 15), label=(21, 16, "UNDER"), pixels=a), dict(index=5, at=(27, 19), label=(24, 20, "OVER"), pixels=b)]
    return {"corners": corners, "overlap": over, "overlap reversed": over[::-1],
            "label outside": [dict(index=7, at=(3, 4), label=(-8, -2, "LEFT AND ABOVE 0123456789"), pixels=a),
                              dict(index=6, at=(30, 20), label=(width - 11, height - 3, "RIGHT AND BELOW"), pixels=b)],
            "no label": [dict(index=3, at=(5, 6), label=None, pixels=b), dict(index=4, at=(25, 6), label=(0, 0, ""), pixels=a)]}
