"""The re-save ahead of the frame as far as it can be checked without a GPU: the entry points are exported, declared and
prototyped, and the folder driver's `resave_ahead` argument is checked before any device work."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("icelk_upload_jpeg_file_async_resave", "icelk_jpeg_async_finish_file", "icelk_jpeg_crop_fwd_device_coefficients")


def test_abi_names_the_entry_points():
    from iceberg_tracking_code_amd import _lib as L
    lib = L.load()
    text = open(os.path.join(ROOT, "include", "icelk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(icelk_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    # the start call takes what the plain one takes, plus quality and want_file; finish_file what a crop job's finish takes
    plain, resave = L.SIGNATURES["icelk_upload_jpeg_file_async"], L.SIGNATURES["icelk_upload_jpeg_file_async_resave"]
    assert resave[0] == plain[0] and resave[1][:len(plain[1])] == plain[1] and len(resave[1]) == len(plain[1]) + 2
    assert L.SIGNATURES["icelk_jpeg_async_finish_file"] == L.SIGNATURES["icelk_jpeg_crop_finish"]


def _names(n):
    return ["/nowhere/20190724-10%02d00.jpg" % k for k in range(n)]


DEVICE = dict(decoder="device", huffman="device")


@pytest.mark.parametrize("kw", [dict(resave="reference"), dict(pipeline=True, **DEVICE), dict(pipeline=False, resave="reference", **DEVICE),
                                dict(pipeline=True, resave=None, save_crops="/nowhere/crops", **DEVICE), dict()])
def test_resave_ahead_needs_pipeline_and_resave(kw):
    """no file of the list exists and no device is touched: the argument check comes first"""
    from iceberg_tracking_code_amd import track_image_sequence
    with pytest.raises(ValueError):
        track_image_sequence(_names(9), "/nowhere/out", 2, 60, resave_ahead=True, **kw)


@pytest.mark.parametrize("kw", [dict(resave="reference"), dict(resave=75, save_crops="/nowhere/crops")])
def test_without_resave_ahead_the_pipeline_refuses_as_before(kw):
    from iceberg_tracking_code_amd import track_image_sequence
    with pytest.raises(ValueError):
        track_image_sequence(_names(9), "/nowhere/out", 2, 60, pipeline=True, **DEVICE, **kw)
    with pytest.raises(ValueError):
        track_image_sequence(_names(9), "/nowhere/out", 2, 60, pipeline=True, resave_ahead=False, **DEVICE, **kw)


def test_resave_ahead_checks_the_other_arguments_first():
    from iceberg_tracking_code_amd import track_image_sequence
    with pytest.raises(ValueError):
        track_image_sequence(_names(9), "/nowhere/out", 2, 60, pipeline=True, resave="best", resave_ahead=True, **DEVICE)
    with pytest.raises(ValueError):
        track_image_sequence(_names(9), "/nowhere/out", 2, 60, pipeline=True, resave="reference", resave_ahead=True, n_slots=4, **DEVICE)
    with pytest.raises(ValueError):
        track_image_sequence(_names(9), "/nowhere/out", 2, 60, pipeline=True, resave="reference", resave_ahead=True, decoder="pil")


def test_resave_ahead_of_a_short_list_returns_nothing():
    from iceberg_tracking_code_amd import track_image_sequence
    for n in (0, 1, 2):
        assert track_image_sequence(_names(n), "/nowhere/out", 2, 60, pipeline=True, resave="reference", resave_ahead=True, **DEVICE) == []
