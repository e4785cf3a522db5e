"""GPU: the fused crop-and-forward kernel (csrc/k_jpeg_fwd.hip: k_jpeg_crop_fwd -- the crop box of a decoded file's planes
straight to the re-saved file's coefficients) through its test entry, against `read_jpeg` of the file Pillow's
`Image.open(f).crop(box).save(out)` writes.  Every int16 of the padded grid is compared, dummy blocks included; the cases
are jpeg_crop_fwd_cases.py's (crop sizes, heights mod 16, origin parities, boxes flush with every true image edge, three
samplings, a source whose chroma planes libjpeg replicates, three qualities)."""
import numpy as np
import pytest

import jpeg_crop_fwd_cases as cc

pytestmark = pytest.mark.gpu


def _groups():
    out = {}
    for case in cc.cases():
        out.setdefault(case[0].split("-")[0], []).append(case)
    return out


GROUPS = _groups()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_f1_fused_coefficients_equal_pillows(ctx, group):
    from iceberg_tracking_code_amd import read_jpeg
    for label, data, size, box, q in GROUPS[group]:
        want = read_jpeg(cc.pillow_crop_file(data, box, q)).coef
        got = ctx.jpeg_crop_fwd_device_coefficients(data, cc.crop4(size, box), 75 if q is None else q)
        assert got.shape == want.shape, (label, got.shape, want.shape)
        assert np.array_equal(got, want), (label, int(np.count_nonzero(got != want)))


def test_f1_equals_the_two_kernel_chain(ctx):
    """the same coefficients as the output kernel followed by the forward kernel leave (icelk_upload_jpeg_file_resave), read
    back through the file both would write"""
    data, size = cc.source("420"), (cc.W, cc.H)
    for box in ((3, 4, 272, 33), (cc.W - 200, cc.H - 9, 200, 9)):
        crop = cc.crop4(size, box)
        ctx.upload_jpeg_file(0, data, 4, crop, resave="reference")
        chain = ctx.jpeg_resave_file()
        ctx.jpeg_crop_fwd_device_coefficients(data, crop)
        assert ctx.jpeg_resave_file() == chain == cc.pillow_crop_file(data, box), box


def test_f1_rejected_calls(ctx):
    data, size = cc.source("420"), (cc.W, cc.H)
    for bad in (cc.crop4(size, (0, 0, 2, 9)), (-1, 0, 0, 0), (cc.W, 0, 0, 0)):
        with pytest.raises(ValueError):
            ctx.jpeg_crop_fwd_device_coefficients(data, bad)
    for q in (0, 101):
        with pytest.raises(ValueError):
            ctx.jpeg_crop_fwd_device_coefficients(data, None, q)
    with pytest.raises(ValueError):
        ctx.jpeg_crop_fwd_device_coefficients(b"not a JPEG file")
