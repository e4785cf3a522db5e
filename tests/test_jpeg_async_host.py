"""The asynchronous JPEG ingest as far as it can be checked without a GPU: the three entry points are exported, declared
and prototyped, and the folder driver's `pipeline` argument is checked before any device work."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("icelk_upload_jpeg_file_async", "icelk_jpeg_async_poll", "icelk_jpeg_async_finish")


def test_abi_names_the_async_entry_points():
    from iceberg_tracking_code_amd import _lib as L
    lib = L.load()
    text = open(os.path.join(ROOT, "include", "icelk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(icelk_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    # the start call takes what icelk_upload_jpeg_file takes
    assert L.SIGNATURES["icelk_upload_jpeg_file_async"] == L.SIGNATURES["icelk_upload_jpeg_file"]


def _names(n):
    return ["/nowhere/20190724-10%02d00.jpg" % k for k in range(n)]


@pytest.mark.parametrize("kw", [dict(decoder="pil"), dict(decoder="device", huffman="host"), dict(decoder="pil", huffman="host")])
def test_pipeline_needs_the_device_decoder(kw):
    """no file of the list exists and no device is touched: the argument check comes first"""
    from iceberg_tracking_code_amd import track_image_sequence
    with pytest.raises(ValueError):
        track_image_sequence(_names(9), "/nowhere/out", 2, 60, pipeline=True, **kw)


def test_pipeline_slots_are_checked():
    from iceberg_tracking_code_amd import track_image_sequence
    with pytest.raises(ValueError):
        track_image_sequence(_names(9), "/nowhere/out", 2, 60, pipeline=True, decoder="device", huffman="device", n_slots=4)


def test_pipeline_of_a_short_list_returns_nothing():
    from iceberg_tracking_code_amd import track_image_sequence
    for n in (0, 1, 2):
        assert track_image_sequence(_names(n), "/nowhere/out", 2, 60, pipeline=True, decoder="device", huffman="device") == []
