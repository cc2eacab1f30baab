"""Host side of the ragged-batch pre/post-processing (csrc/prepost_batch.hip, omnidata_amd/preprocess.py): the packed pixel
buffer, the argument checks of the entry points (they return before anything touches a GPU) and the colormap index rule."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

from omnidata_amd import preprocess as pp

INVALID = -1
PTR = 0x10000   # a non-null "device pointer": an argument check must reject the call before it is ever used


@pytest.fixture(scope="module")
def lib(built_lib):
    from omnidata_amd.engine import load_library
    return load_library()


def test_pack_images_offsets_alignment_and_descriptors():
    rng = np.random.default_rng(0)
    arrays = [rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), rng.integers(0, 256, (3, 3), dtype=np.uint8),
              rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), rng.integers(0, 256, (4, 16, 1), dtype=np.uint8)]
    images = [Image.fromarray(arrays[0]), Image.fromarray(arrays[1]), arrays[2], arrays[3]]
    buf, descs = pp.pack_images(images)
    assert buf.dtype.is_floating_point is False and buf.dim() == 1 and buf.element_size() == 1
    assert C.sizeof(pp.ImageDesc) == 24 and len(descs) == 4
    flat = buf.numpy()
    end = 0
    for d, a in zip(descs, arrays):
        a3 = a if a.ndim == 3 else a[:, :, None]
        assert (d.H, d.W, d.C) == a3.shape and d.row_stride_bytes == d.W * d.C
        assert d.offset % 16 == 0 and d.offset >= end and d.offset - end < 16   # aligned, in order, no more padding than that
        end = d.offset + a3.size
        assert np.array_equal(flat[d.offset:end].reshape(a3.shape), a3)
    assert end <= flat.size
    assert [d.offset for d in descs] == [0, 112, 128, 144]
    with pytest.raises(ValueError):
        pp.pack_images([np.zeros((4, 4, 2), np.uint8)])
    with pytest.raises(ValueError):
        pp.pack_images([np.zeros((4, 4, 3), np.float32)])


def test_batch_supported_routes_other_modes_and_sizes_to_pil():
    assert pp.batch_supported(Image.new("RGB", (50, 40)), 64) and pp.batch_supported(Image.new("L", (50, 40)), 64)
    assert not pp.batch_supported(Image.new("RGBA", (50, 40)), 64)
    assert pp.batch_supported(np.zeros((2048, 3000, 3), np.uint8), 64)
    assert not pp.batch_supported(np.zeros((2049, 3000, 3), np.uint8), 64)      # shorter side 32 * S + 1
    assert not pp.batch_supported(np.zeros((16, 16385), np.uint8), 64)


def _desc(H=70, W=90, Cn=3, stride=None, offset=0):
    return pp.ImageDesc(offset, H, W, Cn, W * Cn if stride is None else stride)


def _pre(lib, descs, B=None, S=64, pixels=PTR, x=PTR, ws=PTR, ws_bytes=1 << 40, descs_null=False):
    arr = (pp.ImageDesc * max(len(descs), 1))(*descs)
    return lib.dptx_preprocess_u8_batch(pixels, None if descs_null else C.addressof(arr), len(descs) if B is None else B, S, 0, x,
                                        ws, ws_bytes, None)


def test_preprocess_batch_rejects_bad_arguments_without_a_gpu(lib):
    good = _desc()
    assert _pre(lib, [good], B=0) == INVALID
    assert _pre(lib, [good], B=4097) == INVALID
    assert _pre(lib, [_desc(Cn=2)]) == INVALID
    assert _pre(lib, [_desc(Cn=4)]) == INVALID
    assert _pre(lib, [_desc(stride=90 * 3 - 1)]) == INVALID
    assert _pre(lib, [good], S=48) == INVALID
    assert _pre(lib, [good], S=2048) == INVALID
    assert _pre(lib, [good], S=0) == INVALID
    assert _pre(lib, [_desc(H=32 * 64 + 1, W=32 * 64 + 1)]) == INVALID          # shorter side = 32 * S + 1
    assert _pre(lib, [_desc(H=32 * 64 + 1, W=4000)]) == INVALID
    assert _pre(lib, [_desc(H=0)]) == INVALID
    assert _pre(lib, [_desc(W=16385, H=64)]) == INVALID
    assert _pre(lib, [_desc(offset=-16)]) == INVALID
    assert _pre(lib, [good, _desc(Cn=2)]) == INVALID                            # any image of the batch
    assert _pre(lib, [good], pixels=None) == INVALID
    assert _pre(lib, [good], x=None) == INVALID
    assert _pre(lib, [good], ws=None) == INVALID
    assert _pre(lib, [good], descs_null=True) == INVALID
    assert _pre(lib, [good], ws_bytes=17664 * 64 - 1) == INVALID                # smaller than the workspace it reports


def test_workspace_sizes_are_reported_on_the_host(lib):
    n = C.c_int64()
    assert lib.dptx_preprocess_batch_workspace_bytes(1, 64, C.byref(n)) == 0 and n.value == 17664 * 64
    assert lib.dptx_preprocess_batch_workspace_bytes(4096, 384, C.byref(n)) == 0 and n.value == 17664 * 384
    for B, S in ((0, 64), (4097, 64), (1, 48), (1, 2048), (1, 16)):
        assert lib.dptx_preprocess_batch_workspace_bytes(B, S, C.byref(n)) == INVALID
    assert lib.dptx_preprocess_batch_workspace_bytes(1, 64, None) == INVALID
    assert lib.dptx_colorize_workspace_bytes(3, 512 * 512, C.byref(n)) == 0 and n.value == 512 * 3
    for B, N in ((0, 16), (1, 0), (65536, 16), (1, (1 << 30) + 1)):
        assert lib.dptx_colorize_workspace_bytes(B, N, C.byref(n)) == INVALID
    assert lib.dptx_colorize_workspace_bytes(1, 16, None) == INVALID


def test_other_entry_points_reject_bad_arguments_without_a_gpu(lib):
    ks = C.c_int32()
    cd = lib.dptx_resample_coeffs_device
    assert cd(0, 64, PTR, PTR, 1 << 30, C.byref(ks), None) == INVALID
    assert cd(64, 0, PTR, PTR, 1 << 30, C.byref(ks), None) == INVALID
    assert cd(100, 64, None, PTR, 1 << 30, C.byref(ks), None) == INVALID
    assert cd(100, 64, PTR, None, 1 << 30, C.byref(ks), None) == INVALID
    assert cd(100, 64, PTR, PTR, 1 << 30, None, None) == INVALID
    assert cd(640, 64, PTR, PTR, 64 * 21 - 1, C.byref(ks), None) == INVALID and ks.value == 21   # capacity too small; ksize told
    for fn in (lib.dptx_postprocess_normal_u8_batch, lib.dptx_postprocess_depth_batch):
        assert fn(None, 1, 64, PTR, None) == INVALID
        assert fn(PTR, 1, 64, None, None) == INVALID
        assert fn(PTR, 0, 64, PTR, None) == INVALID
        assert fn(PTR, 1, 0, PTR, None) == INVALID
        assert fn(PTR, 65536, 64, PTR, None) == INVALID
    col = lib.dptx_colorize_u8_batch
    assert col(None, PTR, 1, 16, PTR, PTR, 1 << 20, None) == INVALID
    assert col(PTR, None, 1, 16, PTR, PTR, 1 << 20, None) == INVALID
    assert col(PTR, PTR, 1, 16, None, PTR, 1 << 20, None) == INVALID
    assert col(PTR, PTR, 1, 16, PTR, None, 1 << 20, None) == INVALID
    assert col(PTR, PTR, 0, 16, PTR, PTR, 1 << 20, None) == INVALID
    assert col(PTR, PTR, 1, 0, PTR, PTR, 1 << 20, None) == INVALID
    assert col(PTR, PTR, 2, 16, PTR, PTR, 1023, None) == INVALID                # workspace smaller than 512 * B


def test_lut_index_rule_equals_matplotlibs_float_path():
    """plt.imsave's float path (normalise, colormap call, *255 -> uint8) is the 256-entry table indexed by
    min(int(n * 256), 255): what dptx_colorize_u8_batch computes from the caller's table."""
    o = np.linspace(0, 1, 4097, dtype=np.float32).reshape(1, -1)
    want = pp.colorize_viridis(o)
    lut = pp.viridis_lut()
    assert lut.shape == (256, 4) and lut.dtype == np.uint8
    lo, hi = np.float32(o.min()), np.float32(o.max())
    n = (o - lo) / (hi - lo)
    assert n.dtype == np.float32
    idx = np.minimum((n * np.float32(256)).astype(np.int64), 255)
    assert idx.min() == 0 and idx.max() == 255
    assert np.array_equal(lut[idx], want)
