"""GPU: the forms of JPEG ingest agree with each other.  Every mode is pinned against Pillow elsewhere (test_gpu_jpeg*.py);
here one tiny photo goes through every upload into the slots of one handle and the level-0 images must be equal, with and
without the re-save, with and without the host decoder taking the file -- so a slip in a step the forms share
(csrc/abi_jpeg_ingest.hip) shows in seconds.  Every comparison is exact equality."""
import numpy as np
import pytest
from PIL import Image

import jpeg_resave_cases as rc

pytestmark = pytest.mark.gpu

# (size, crop): the 4:2:0 photo with the odd crop, and one whose cropped chroma plane is narrow
CASES = ((rc.PHOTO_SIZE, rc.CROP), ((41, 7), (1, 0, 1, 0)))


@pytest.fixture(scope="module")
def h5():
    from iceberg_tracking_code_amd import Context
    c = Context(256, 128, n_slots=5, max_pts=64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def photos(tmp_path_factory):
    """per case: the file, PIL's pixels, and PIL's pixels of the reference's re-saved crop (camtools.py:64-104)"""
    d = tmp_path_factory.mktemp("forms")
    out = []
    for k, (size, crop) in enumerate(CASES):
        src, dst = str(d / ("%d.jpg" % k)), str(d / ("%d_crop.jpg" % k))
        data = rc.photo_file(size=size)
        with open(src, "wb") as f:
            f.write(data)
        rc.reference_crop_resave(src, dst, crop)
        out.append(dict(data=data, crop=crop, pixels=np.array(Image.open(src)), resaved=np.array(Image.open(dst))))
    return out


def _forms(h5, p, variant, resave):
    """level 0 by form, and the statistics of the two forms that decode the file on the device"""
    from iceberg_tracking_code_amd import read_jpeg
    kw = {} if resave is None else dict(resave=resave)
    got, stats = {}, {}
    h5.upload_bgr(0, p["pixels"], variant, p["crop"], **kw)
    got["upload_bgr"] = h5.download_level(0, 0)
    h5.upload_jpeg(1, read_jpeg(p["data"]), variant, p["crop"], **kw)
    got["upload_jpeg"] = h5.download_level(1, 0)
    h5.upload_jpeg_file(2, p["data"], variant, p["crop"], **kw)
    got["upload_jpeg_file"] = h5.download_level(2, 0)
    stats["sync"] = h5.jpeg_huff_stats()
    if resave is None:
        h5.upload_jpeg_file_async(3, p["data"], variant, p["crop"])
        stats["async"] = h5.jpeg_async_finish(3)
        got["upload_jpeg_file_async"] = h5.download_level(3, 0)
    # the Pillow oracle through the plain upload
    left, top, right, bottom = p["crop"]
    px = p["pixels"]
    h5.upload_bgr(4, px[top:px.shape[0] - bottom, left:px.shape[1] - right] if resave is None else p["resaved"], variant)
    return got, stats, h5.download_level(4, 0)


def _check_equal(got, want, what):
    for form, img in got.items():
        assert img.shape == want.shape and np.array_equal(img, want), (form,) + what + (int(np.count_nonzero(img != want)),)


@pytest.mark.parametrize("bounded", [False, True], ids=["device", "host_takes_the_file"])
def test_forms_agree(h5, photos, bounded):
    """bounded: a work bound no file meets (one hop, one round), so the host decoder takes the file in the synchronous and
    in the asynchronous form."""
    h5.jpeg_huff_config(max_hops=1, max_rounds=1) if bounded else h5.jpeg_huff_config()
    try:
        for p in photos:
            for variant in (3, 4):
                for resave in (None, "reference"):
                    got, stats, want = _forms(h5, p, variant, resave)
                    _check_equal(got, want, (p["crop"], variant, resave))
                    for form, st in stats.items():
                        assert (st["fallback"] != 0) == bounded, (form, p["crop"], variant, resave, st)
    finally:
        h5.jpeg_huff_config()


# What each synchronous entry point launches from the JPEG group, as prof_table counts it (one per ProfScope), read from the
# code before the shared steps were named: the Huffman decoder has one scope around the rounds and one around scan, write
# and DC pass; the transform and the output kernel one each.  A file that decodes on the device; a 3-component one.
LAUNCHES = {
    "upload_jpeg": dict(jpeg_idct=1, jpeg_out=1),
    "jpeg_decode_rgb": dict(jpeg_idct=1, jpeg_out=1),
    "upload_jpeg_file": dict(jpeg_huff=2, jpeg_idct=1, jpeg_out=1),
    "jpeg_decode_rgb_file": dict(jpeg_huff=2, jpeg_idct=1, jpeg_out=1),
    "jpeg_device_coefficients": dict(jpeg_huff=2),
}
# The forms that put a file in flight (one scope around all rounds and phases, one per other step; the budgeted coder's six
# scopes when a file is wanted), counted over start and finish together.  Measured on commit cbed01b, before these forms
# were given one driver (csrc/abi_jpeg_job.hip), never taken from that driver.
_CODER = dict(jpeg_enc_count=1, jpeg_enc_scan=2, jpeg_enc_pack_budget=1, jpeg_enc_ff_budget=1, jpeg_enc_stuff_budget=1)
_SLOT_RESAVE = dict(jpeg_huff=1, jpeg_idct=2, jpeg_crop_fwd=1, jpeg_out=1, jpeg_crop_verdict=1)
LAUNCHES.update({
    "upload_jpeg_file_async": dict(jpeg_huff=1, jpeg_idct=1, jpeg_out=1),
    "upload_jpeg_file_async_resave": _SLOT_RESAVE,
    "upload_jpeg_file_async_crop_file": dict(_SLOT_RESAVE, **_CODER),
    "jpeg_crop": dict(jpeg_huff=1, jpeg_idct=1, jpeg_crop_rgb=1, jpeg_fwd=1, jpeg_crop_verdict=1, **_CODER),
})


def _in_flight(h5, data, crop):
    def slot_form(**kw):
        h5.upload_jpeg_file_async(3, data, 4, crop, **kw)
        if kw.get("crop_file"):
            assert h5.jpeg_async_finish_file(3)[1]["route"] == "device"
        else:
            assert h5.jpeg_async_finish(3)["fallback"] == 0

    def crop_form():
        assert h5.jpeg_crop_finish(h5.jpeg_crop_start(data, crop, "reference"))[1]["route"] == "device"

    return {
        "upload_jpeg_file_async": slot_form,
        "upload_jpeg_file_async_resave": lambda: slot_form(resave="reference"),
        "upload_jpeg_file_async_crop_file": lambda: slot_form(resave="reference", crop_file=True),
        "jpeg_crop": crop_form,
    }


def test_launches_per_entry_point(h5, photos):
    from iceberg_tracking_code_amd import read_jpeg
    data = photos[0]["data"]
    j = read_jpeg(data)
    calls = {
        "upload_jpeg": lambda: h5.upload_jpeg(0, j, 4),
        "jpeg_decode_rgb": lambda: h5.jpeg_decode_rgb(j),
        "upload_jpeg_file": lambda: h5.upload_jpeg_file(0, data, 4),
        "jpeg_decode_rgb_file": lambda: h5.jpeg_decode_rgb_file(data),
        "jpeg_device_coefficients": lambda: h5.jpeg_device_coefficients(data),
    }
    calls.update(_in_flight(h5, data, photos[0]["crop"]))
    h5.jpeg_huff_config()
    for name, want in LAUNCHES.items():
        h5.prof_reset()
        h5.prof_enable(True)
        try:
            calls[name]()
        finally:
            h5.prof_enable(False)
        got = {k: v["launches"] for k, v in h5.prof_table().items() if k.startswith("jpeg_")}
        print(name, got)
        assert got == want, name
    h5.prof_reset()
