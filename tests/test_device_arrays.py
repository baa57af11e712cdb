"""The pure-Python side of the device inputs (capi.device_array_info / device_frames_args and the argument shaping of the
Handle.*_device methods): ``__cuda_array_interface__`` is read off a fake object, nothing calls the library, no GPU needed."""
import importlib

import numpy as np
import pytest

capi = importlib.import_module("slam-eds_amd.capi")

H, W = 37, 50
PTR = 0x7F0000001000


class Fake:
    """an object that only has the interface: shape, numpy dtype, byte strides (None: dense)"""

    def __init__(self, shape, dtype, strides=None, ptr=PTR, **extra):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=np.dtype(dtype).str, data=(ptr, False), strides=strides,
                                             version=3, **extra)


def test_dense_frames_fp32_and_fp64():
    assert capi.device_frames_args(Fake((5, H, W), np.float32), H, W) == (PTR, 5, capi.IMG_F32, H * W, W)
    assert capi.device_frames_args(Fake((5, H, W), np.float64), H, W) == (PTR, 5, capi.IMG_F64, H * W, W)
    # explicit dense byte strides say the same as None
    assert capi.device_frames_args(Fake((5, H, W), np.float64, (H * W * 8, W * 8, 8)), H, W) == (PTR, 5, capi.IMG_F64, H * W, W)


def test_a_single_frame_may_be_two_dimensional():
    assert capi.device_frames_args(Fake((H, W), np.float32), H, W) == (PTR, 1, capi.IMG_F32, H * W, W)
    # one pitched frame: the frame stride is whatever covers it
    assert capi.device_frames_args(Fake((H, W), np.float64, ((W + 3) * 8, 8)), H, W) == (PTR, 1, capi.IMG_F64, (H - 1) * (W + 3) + W, W + 3)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pitched_frames_byte_strides_become_elements(dtype):
    it = np.dtype(dtype).itemsize
    row, frame = W + 3, H * (W + 3) + 5
    got = capi.device_frames_args(Fake((33, H, W), dtype, (frame * it, row * it, it)), H, W)
    assert got == (PTR, 33, capi.IMG_F32 if it == 4 else capi.IMG_F64, frame, row)


def test_raw_tuple_is_accepted():
    assert capi.device_frames_args((PTR, (2, H, W), None, np.float32), H, W) == (PTR, 2, capi.IMG_F32, H * W, W)
    assert capi.device_frames_args((PTR, (2, H, W), (H * (W + 1) * 4, (W + 1) * 4, 4), "float32"), H, W) == (PTR, 2, capi.IMG_F32, H * (W + 1), W + 1)


def test_rejected_before_the_library_is_called():
    with pytest.raises(ValueError, match="contiguous"):          # a transposed view: the last stride is a row
        capi.device_frames_args(Fake((3, H, W), np.float32, (H * W * 4, 4, H * 4)), H, W)
    with pytest.raises(ValueError, match="float16"):
        capi.device_frames_args(Fake((3, H, W), np.float16), H, W)
    with pytest.raises(ValueError, match="int32"):
        capi.device_frames_args(Fake((3, H, W), np.int32), H, W)
    with pytest.raises(ValueError, match="do not fit"):          # wrong H x W
        capi.device_frames_args(Fake((3, W, H), np.float32), H, W)
    with pytest.raises(ValueError, match="do not fit"):
        capi.device_frames_args(Fake((3, H, W + 1), np.float32), H, W)
    with pytest.raises(ValueError, match="1-dimensional"):       # 1-D where count x H x W is required
        capi.device_frames_args(Fake((3 * H * W,), np.float32), H, W)
    with pytest.raises(ValueError, match="4-dimensional"):
        capi.device_frames_args(Fake((1, 3, H, W), np.float32), H, W)
    with pytest.raises(ValueError, match="whole number"):        # a byte stride that is no multiple of the element
        capi.device_frames_args(Fake((3, H, W), np.float32, (H * W * 4 + 2, W * 4, 4)), H, W)
    with pytest.raises(ValueError, match="rows overlap"):
        capi.device_frames_args(Fake((3, H, W), np.float32, (H * W * 4, (W - 1) * 4, 4)), H, W)
    with pytest.raises(ValueError, match="rows overlap"):        # a vertically flipped view
        capi.device_frames_args(Fake((3, H, W), np.float32, (H * W * 4, -W * 4, 4)), H, W)
    with pytest.raises(ValueError, match="frames overlap"):      # the same frame broadcast over the batch
        capi.device_frames_args(Fake((3, H, W), np.float32, (0, W * 4, 4)), H, W)
    with pytest.raises(ValueError, match="no frame"):
        capi.device_frames_args(Fake((0, H, W), np.float32), H, W)
    with pytest.raises(ValueError, match="without a pointer"):
        capi.device_frames_args(Fake((3, H, W), np.float32, ptr=0), H, W)
    with pytest.raises(ValueError, match="__cuda_array_interface__"):
        capi.device_frames_args(np.zeros((3, H, W), np.float32), H, W)       # host memory is not silently uploaded


def test_array_info_strides_in_elements():
    assert capi.device_array_info(Fake((4, 6), np.float64)) == (PTR, (4, 6), (6, 1), np.dtype(np.float64))
    assert capi.device_array_info(Fake((4, 6, 2), np.uint16, (48, 8, 2))) == (PTR, (4, 6, 2), (24, 4, 1), np.dtype(np.uint16))
    assert capi.device_array_info(Fake((7,), np.uint8)) == (PTR, (7,), (1,), np.dtype(np.uint8))
    with pytest.raises(ValueError, match="different lengths"):
        capi.device_array_info(Fake((4, 6), np.float64, (8,)))


def test_keyframe_rows():
    rows = capi._device_rows
    assert rows(Fake((3, 40, 2), np.float64), 3, 2, "norm_coord") == (PTR, 40, 40)
    assert rows(Fake((3, 40), np.float64), 3, 1, "idp") == (PTR, 40, 40)
    # rows 47 points apart, 40 of them described
    assert rows(Fake((3, 40, 2), np.float64, (47 * 16, 16, 8)), 3, 2, "grad") == (PTR, 40, 47)
    assert rows(Fake((3, 40), np.float64, (47 * 8, 8)), 3, 1, "weights") == (PTR, 40, 47)
    assert rows(Fake((40, 2), np.float64), 1, 2, "norm_coord") == (PTR, 40, 40)        # one alignment without the leading axis
    with pytest.raises(ValueError, match="float64"):
        rows(Fake((3, 40, 2), np.float32), 3, 2, "norm_coord")
    with pytest.raises(ValueError, match="count x S"):
        rows(Fake((2, 40, 2), np.float64), 3, 2, "norm_coord")
    with pytest.raises(ValueError, match="contiguous"):
        rows(Fake((3, 40, 2), np.float64, (40 * 32, 32, 8)), 3, 2, "norm_coord")         # every second point
    with pytest.raises(ValueError, match="overlap"):
        rows(Fake((3, 40), np.float64, (39 * 8, 8)), 3, 1, "idp")
    with pytest.raises(ValueError, match="overlap"):
        rows(Fake((3, 40, 2), np.float64, (41 * 8, 16, 8)), 3, 2, "norm_coord")          # half a point


def test_stream_argument():
    class S:
        cuda_stream = 0x1234

    class Null:
        cuda_stream = 0

    assert capi._stream_ptr(None) is None and capi._stream_ptr(0) is None and capi._stream_ptr(Null()) is None
    assert capi._stream_ptr(S()) == 0x1234 and capi._stream_ptr(77) == 77


def test_is_device_array():
    assert capi.is_device_array(Fake((H, W), np.float32)) and not capi.is_device_array(np.zeros((H, W)))
