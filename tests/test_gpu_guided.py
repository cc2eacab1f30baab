"""Guided upsampling on the device (csrc/guided.hip, dptx_postprocess_guided_batch, pp.guided_outputs_gpu) against the restatement
of tests/guided_restatement.py on the small cases of tests/guided_cases.py.

fp32 outputs: max |got - fp64| <= 4 * E, with E the largest |fp32 restatement - fp64 restatement| of the same call, computed here
from the two restatements alone; the factor 4 allows for another exp and another grouping of the sums on the device.  Dropping
one ring of taps moves the median pixel by about 0.06, so anything structural fails by five orders of magnitude.
uint8 outputs: no byte more than one level from the fp64 restatement's, at most 0.1 % of a call's bytes different
(tests/test_guided_host.py checks that the fp32 restatement itself stays under a quarter of that on these inputs).
Measured (MI355X, profiles/guided_parity.md): the largest err / E of the 108 fp32 runs is 2.13 (a renormalised call), 106 are at
or below 1.00; of the uint8 runs none has more than one differing byte in a call (4 bytes in all, one level each)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from omnidata_amd import preprocess as pp
from guided_cases import CALLS, RADII, SIGMA_RANGES, SIGMA_SPACE, inputs, pack_guides, restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMAL_U8, NORMAL_F32, DEPTH_F32, DEPTH_RGBA, RENORM = 1, 2, 3, 4, 16
INVALID = -1


def _lib():
    from omnidata_amd.engine import load_library
    return load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _device_inputs(name, Cn):
    """-> (S, G_lo, pixels, guide descriptors) on the device; the guides at odd offsets, some grey, some with padded rows."""
    S, G_lo, guides = inputs(name, Cn)
    pixels, gdescs = pack_guides(name, guides)
    descs = (pp.ImageDesc * len(gdescs))(*[pp.ImageDesc(*d) for d in gdescs])
    return S.to(DEV), G_lo.to(DEV), torch.from_numpy(pixels).to(DEV), descs


@functools.lru_cache(maxsize=None)
def _got(name, mode, renorm=False, radius=2, sigma_range=0.25):
    Cn = 3 if mode.startswith("normal") else 1
    S, G_lo, pixels, descs = _device_inputs(name, Cn)
    outs = pp.guided_outputs_gpu(S, G_lo, pixels, descs, CALLS[name][2], mode, renorm, radius, SIGMA_SPACE, sigma_range)
    return tuple(o.cpu() for o in outs)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_fp32_outputs_are_within_four_times_the_fp32_restatements_own_error(name):
    for radius in RADII:
        for sigma_range in SIGMA_RANGES:
            for mode, renorm in (("normal_f32", False), ("normal_f32", True), ("depth_f32", False)):
                r64 = restated(name, mode, renorm, radius, sigma_range, torch.float64)
                r32 = restated(name, mode, renorm, radius, sigma_range, torch.float32)
                E = max(float((a.double() - b).abs().max()) for a, b in zip(r32, r64))
                got = _got(name, mode, renorm, radius, sigma_range)
                assert [tuple(g.shape) for g in got] == [tuple(r.shape) for r in r64]
                err = max(float((a.double() - b).abs().max()) for a, b in zip(got, r64))
                same = all(torch.equal(a, b) for a, b in zip(got, r32))
                print(f"guided parity {name} R={radius} sr={sigma_range} {mode}{'+renorm' if renorm else ''}: E {E:.3e} err {err:.3e} "
                      f"ratio {err / E:.2f} bit-identical-to-fp32-restatement {same}")
                assert err <= 4 * E


@pytest.mark.parametrize("name", sorted(CALLS))
def test_uint8_outputs_are_within_one_level_and_differ_in_at_most_a_thousandth_of_the_bytes(name):
    for radius in RADII:
        for sigma_range in SIGMA_RANGES:
            for renorm in (False, True):
                r64 = restated(name, "normal_u8", renorm, radius, sigma_range, torch.float64)
                got = _got(name, "normal_u8", renorm, radius, sigma_range)
                assert all(g.dtype == torch.uint8 and g.shape == r.shape for g, r in zip(got, r64))
                diff = torch.cat([(a.int() - b.int()).abs().reshape(-1) for a, b in zip(got, r64)])
                print(f"guided parity {name} R={radius} sr={sigma_range} normal_u8{'+renorm' if renorm else ''}: "
                      f"{int((diff > 0).sum())} of {diff.numel()} bytes differ, max {int(diff.max())}")
                assert int(diff.max()) <= 1
                assert int((diff > 0).sum()) <= 0.001 * diff.numel()


@pytest.mark.parametrize("name", sorted(CALLS))
def test_depth_rgba_is_viridis_of_the_calls_own_depth_f32_values(name):
    for radius in RADII:
        for i, (rgba, f32) in enumerate(zip(_got(name, "depth_rgba", False, radius), _got(name, "depth_f32", False, radius))):
            assert rgba.shape == (*CALLS[name][2][i], 4) and rgba.dtype == torch.uint8
            assert np.array_equal(rgba.numpy(), pp.colorize_viridis(f32.numpy())), (radius, i)


@pytest.mark.parametrize("mode", ["normal_u8", "normal_f32", "depth_f32", "depth_rgba"])
def test_a_second_call_and_an_image_alone_give_the_bits_of_the_batch_and_33_cross_a_chunk(mode):
    name = "5x7"
    Cn = 3 if mode.startswith("normal") else 1
    S, G_lo, pixels, descs = _device_inputs(name, Cn)
    sizes = CALLS[name][2]
    got = _got(name, mode)
    again = pp.guided_outputs_gpu(S, G_lo, pixels, descs, sizes, mode, False, 2, SIGMA_SPACE, 0.25)
    for i, size in enumerate(sizes):
        assert torch.equal(again[i].cpu(), got[i]), i
        one = (pp.ImageDesc * 1)(descs[i])
        alone = pp.guided_outputs_gpu(S[i:i + 1], G_lo[i:i + 1], pixels, one, [size], mode, False, 2, SIGMA_SPACE, 0.25)[0]
        assert torch.equal(alone.cpu(), got[i]), i
    idx = [i % 3 for i in range(33)]
    many = pp.guided_outputs_gpu(S[idx].contiguous(), G_lo[idx].contiguous(), pixels, (pp.ImageDesc * 33)(*[descs[i] for i in idx]),
                                 [sizes[i] for i in idx], mode, False, 2, SIGMA_SPACE, 0.25)
    for k, i in enumerate(idx):
        assert torch.equal(many[k].cpu(), got[i]), k


def _raw(name, code, params, guard=64, **bad):
    """dptx_postprocess_guided_batch into a buffer of 0xA5 with padded rows and gaps between the outputs -> (return code, buffer,
    mask of the bytes the outputs own, per-output bytes).  `bad` overrides one argument."""
    from omnidata_amd._native import workspace
    base = code & 15
    u8 = base == NORMAL_U8
    Cn = 3 if base in (NORMAL_U8, NORMAL_F32) else 1
    bpp, planes = (3 if u8 else 4), (3 if base == NORMAL_F32 else 1)
    S, G_lo, pixels, gdescs = _device_inputs(name, Cn)
    h, w, sizes = CALLS[name][:3]
    descs = (pp.ImageDesc * len(sizes))()
    off, spans = (1 if u8 else 4), []
    for i, (H, W) in enumerate(sizes):
        stride = W * bpp + ((1, 2, 3, 5)[i % 4] if u8 else 4 * (1 + i % 3))
        descs[i] = pp.ImageDesc(off, H, W, 3, stride)
        spans.append((off, planes * H, W * bpp, stride))
        off += planes * H * stride + ((3, 1, 6)[i % 3] if u8 else 8)
    buf = torch.full((off + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    lut = torch.from_numpy(pp.viridis_lut()).to(DEV)
    ws = workspace("dptx_postprocess_guided_workspace_bytes", torch.device(DEV), (len(sizes), DEPTH_RGBA), "unsupported")
    a = dict(y=S.data_ptr(), lo=G_lo.data_ptr(), B=len(sizes), C=Cn, h=h, w=w, pixels=pixels.data_ptr(), guides=C.addressof(gdescs),
             outs=C.addressof(descs), params=None if params is None else C.addressof(params), mode=code, out=buf.data_ptr(), lut=lut.data_ptr(), ws=ws.data_ptr(),
             ws_bytes=ws.numel())
    a.update(bad)
    rc = _lib().dptx_postprocess_guided_batch(a["y"], a["lo"], a["B"], a["C"], a["h"], a["w"], a["pixels"], a["guides"], a["outs"],
                                              a["params"], a["mode"], a["out"], a["lut"], a["ws"], a["ws_bytes"], _stream())
    host = buf.cpu().numpy()
    owned = np.zeros(host.shape, dtype=bool)
    outs = []
    for o, rows, rowbytes, stride in spans:
        idx = o + np.arange(rows)[:, None] * stride + np.arange(rowbytes)[None, :]
        owned[idx] = True
        outs.append(host[idx])
    return rc, host, owned, outs


@pytest.mark.parametrize("mode,code", [("normal_u8", NORMAL_U8), ("normal_u8", NORMAL_U8 | RENORM), ("normal_f32", NORMAL_F32),
                                       ("depth_f32", DEPTH_F32), ("depth_rgba", DEPTH_RGBA)])
def test_bytes_between_padded_rows_and_between_outputs_are_untouched(mode, code):
    """W = 37, 65, 129: 3 * W is no multiple of 4 and the rows start at every byte alignment."""
    for name in ("5x7", "40x48"):
        rc, host, owned, outs = _raw(name, code, pp.GuidedParams(2, SIGMA_SPACE, 0.25))
        assert rc == 0
        assert (host[~owned] == 0xA5).all()
        for i, (o, t) in enumerate(zip(outs, _got(name, mode, bool(code & RENORM)))):
            assert np.array_equal(o.reshape(-1), t.contiguous().view(torch.uint8).numpy().reshape(-1)), (name, i)   # padded == tight


def test_invalid_arguments_return_invalid_without_a_launch():
    name, good = "5x7", pp.GuidedParams(2, 1.0, 0.1)
    sizes = CALLS[name][2]
    _, _, _, gdescs = _device_inputs(name, 3)

    def guides(i, **change):
        arr = (pp.ImageDesc * len(sizes))(*gdescs)
        for k, v in change.items():
            setattr(arr[i], k, v)
        return arr

    def rejected(code=NORMAL_F32, params=good, **bad):
        rc, host, _, _ = _raw(name, code, params, **bad)
        return rc == INVALID and bool((host == 0xA5).all())          # nothing was written: nothing was launched

    assert _raw(name, NORMAL_F32, good)[0] == 0
    for params in (pp.GuidedParams(0, 1.0, 0.1), pp.GuidedParams(4, 1.0, 0.1), pp.GuidedParams(-1, 1.0, 0.1),
                   pp.GuidedParams(2, 0.0, 0.1), pp.GuidedParams(2, -1.0, 0.1), pp.GuidedParams(2, 1.0, 0.0),
                   pp.GuidedParams(2, 1.0, -0.1), pp.GuidedParams(2, float("nan"), 0.1), pp.GuidedParams(2, 1.0, float("nan")),
                   pp.GuidedParams(2, 1.0, 1e-30), pp.GuidedParams(2, float("inf"), 0.1), pp.GuidedParams(2, 1.0, float("inf"))):
        assert rejected(params=params), (params.radius, params.sigma_space, params.sigma_range)
    for change in (dict(H=sizes[1][0] + 1), dict(W=sizes[1][1] - 1), dict(C=2), dict(C=4), dict(C=0), dict(offset=-1),
                   dict(row_stride_bytes=sizes[1][1] - 1)):
        keep = guides(1, **change)
        assert rejected(guides=C.addressof(keep)), change
    for bad in (dict(B=0), dict(B=4097), dict(C=1), dict(h=0), dict(w=4097), dict(y=None), dict(lo=None), dict(pixels=None),
                dict(guides=None), dict(outs=None), dict(params=None), dict(out=None), dict(mode=0), dict(mode=5),
                dict(mode=DEPTH_F32 | RENORM), dict(mode=NORMAL_F32 | 32)):
        assert rejected(**bad), bad
    assert rejected(code=DEPTH_RGBA, ws=None) and rejected(code=DEPTH_RGBA, lut=None) and rejected(code=DEPTH_RGBA, ws_bytes=16383)
    nbytes = C.c_int64(-1)
    assert _lib().dptx_postprocess_guided_workspace_bytes(3, DEPTH_RGBA, C.byref(nbytes)) == 0 and nbytes.value == 16384
    assert _lib().dptx_postprocess_guided_workspace_bytes(3, NORMAL_U8 | RENORM, C.byref(nbytes)) == 0 and nbytes.value == 0
    assert _lib().dptx_postprocess_guided_workspace_bytes(3, DEPTH_RGBA | RENORM, C.byref(nbytes)) == INVALID
    with pytest.raises(ValueError):
        S, G_lo, pixels, descs = _device_inputs(name, 3)
        pp.guided_outputs_gpu(S, G_lo[:, :, :-1], pixels, descs, sizes, "normal_u8")


def test_the_entry_point_replays_from_a_captured_graph():
    """No hidden allocation or synchronisation: both launches of DEPTH_RGBA capture, and a replay gives the same bits."""
    from omnidata_amd._native import workspace
    name = "5x7"
    S, G_lo, pixels, gdescs = _device_inputs(name, 1)
    h, w, sizes = CALLS[name][:3]
    outs, total = pp.output_layout(sizes, "depth_rgba")
    buf = torch.zeros(total, dtype=torch.uint8, device=DEV)
    lut = torch.from_numpy(pp.viridis_lut()).to(DEV)
    ws = workspace("dptx_postprocess_guided_workspace_bytes", torch.device(DEV), (len(sizes), DEPTH_RGBA), "unsupported")
    params = pp.GuidedParams(2, SIGMA_SPACE, 0.25)

    def run(stream):
        assert _lib().dptx_postprocess_guided_batch(S.data_ptr(), G_lo.data_ptr(), len(sizes), 1, h, w, pixels.data_ptr(),
                                                    C.addressof(gdescs), C.addressof(outs), C.addressof(params), DEPTH_RGBA,
                                                    buf.data_ptr(), lut.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(_stream())
    buf.zero_()
    g.replay()
    torch.cuda.synchronize()
    for o, want in zip(pp._output_views(buf, outs, sizes, "depth_rgba"), _got(name, "depth_rgba")):
        assert torch.equal(o.cpu(), want)


# ------------------------------------------------------------------------------------------------ end to end
E2E = [("a", (70, 90), "RGB"), ("b", (90, 70), "L"), ("c", (64, 64), "RGB"), ("d", (33, 50), "RGBA"), ("e", (120, 300), "RGB")]   # (H, W)


def _folder(path):
    rng = np.random.default_rng(11)
    path.mkdir()
    for stem, (h, w), mode in E2E:
        Image.fromarray(rng.integers(0, 256, (h, w) if mode == "L" else (h, w, len(mode)), dtype=np.uint8), mode).save(path / f"{stem}.png")
    return [str(path / f"{stem}.png") for stem, _, _ in E2E]


@functools.lru_cache(maxsize=None)
def _model(task):
    if task == "unet":
        from omnidata_amd.unet import build_unet
        return build_unet("normal", random_weights=0, dtype="fp16", max_batch=2).to(DEV)
    from omnidata_amd.model import build_model
    return build_model(task, random_weights=0, dtype="bf16", max_batch=2).to(DEV)


@pytest.mark.parametrize("task,full_frame,renorm,guided", [("normal", "aspect", True, True), ("normal", "squash", False, dict(radius=1)),
                                                           ("depth", "aspect", False, dict(radius=3, sigma_range=0.2))])
def test_the_predictor_equals_guided_outputs_gpu_applied_by_hand_to_the_same_forward(tmp_path, task, full_frame, renorm, guided):
    from omnidata_amd.batch_infer import BatchPredictor
    files = _folder(tmp_path / "in")
    model = _model(task)
    bp = BatchPredictor(model, task, batch_size=2, image_size=64, full_frame=full_frame, renormalize=renorm, guided=guided)
    outs = list(bp.predict(files))
    plain = list(BatchPredictor(model, task, batch_size=2, image_size=64, full_frame=full_frame, renormalize=renorm).predict(files))
    mode = "depth_rgba" if task == "depth" else "normal_u8"
    options = {} if guided is True else guided
    for f, (stem, (h, w), _), o, p in zip(files, E2E, outs, plain):
        img = Image.open(f)
        net = (64, 64) if full_frame == "squash" else pp.full_frame_net_size(w, h, 64)[1::-1]
        x = pp.images_to_input_rect_gpu([img], task, net, DEV)
        y = model(x).clamp(0, 1)
        pixels, descs = pp.pack_images([img if img.mode in ("RGB", "L") else img.convert("RGB")])
        lo = x * 0.5 + 0.5 if task == "depth" else x
        want = pp.guided_outputs_gpu(y, lo, pixels.to(DEV), descs, [(h, w)], mode, renorm, **options)[0]
        assert o.is_cuda and o.dtype == torch.uint8 and o.shape == (h, w, 4 if task == "depth" else 3)
        assert torch.equal(o, want), stem
        assert torch.equal(p, pp.resize_outputs_gpu(y, [(h, w)], mode, renorm)[0]), stem      # guided=None: the plain resize, bit for bit
        assert not torch.equal(o, p), stem
    bp.predict_to_dir(files, str(tmp_path / "out"))
    for stem, (h, w), _ in E2E:
        png = Image.open(tmp_path / "out" / f"{stem}_{task}.png")
        assert png.size == (w, h) and np.array_equal(np.asarray(png), outs[[s for s, _, _ in E2E].index(stem)].cpu().numpy()), stem


def test_the_version_1_unet_takes_guided_with_squash(tmp_path):
    from omnidata_amd.batch_infer import BatchPredictor
    files = _folder(tmp_path / "in")
    model = _model("unet")
    outs = list(BatchPredictor(model, "normal", batch_size=2, image_size=128, full_frame="squash", guided=True).predict(files))
    for f, (stem, (h, w), _), o in zip(files, E2E, outs):
        img = Image.open(f)
        x = pp.images_to_input_rect_gpu([img], "normal", (128, 128), DEV)
        y = model(x).clamp(0, 1)
        pixels, descs = pp.pack_images([img if img.mode in ("RGB", "L") else img.convert("RGB")])
        assert torch.equal(o, pp.guided_outputs_gpu(y, x, pixels.to(DEV), descs, [(h, w)], "normal_u8")[0]), stem


def test_demo_cli_guided_writes_the_map_at_the_images_own_size(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    rng = np.random.default_rng(5)
    shapes = (("a", (400, 520)), ("b", (390, 300)))
    for stem, (h, w) in shapes:
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(src / f"{stem}.png")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--task", "normal", "--img_path", str(src), "--output_path", str(out),
                        "--random-weights", "0", "--dtype", "bf16", "--full_frame", "aspect", "--guided"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for stem, (h, w) in shapes:
        png = Image.open(out / f"{stem}_normal.png")
        assert png.size == (w, h) and np.asarray(png).std() > 0
        assert Image.open(out / f"{stem}_rgb.png").size == (w, h)
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--task", "normal", "--img_path", str(src), "--output_path", str(out),
                          "--random-weights", "0", "--guided"], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT),
                         cwd=ROOT, timeout=600)
    assert "--guided needs --full_frame" in bad.stdout


def test_return_pixels_leaves_the_input_unchanged_and_describes_every_image():
    imgs = [Image.fromarray(np.random.default_rng(i).integers(0, 256, s, dtype=np.uint8), m)
            for i, (s, m) in enumerate([((33, 50, 3), "RGB"), ((20, 31, 4), "RGBA"), ((64, 64), "L")])]
    x0 = pp.images_to_input_rect_gpu(imgs, "normal", (64, 96), DEV)
    x, pixels, descs = pp.images_to_input_rect_gpu(imgs, "normal", (64, 96), DEV, return_pixels=True)
    assert torch.equal(x, x0) and pixels.is_cuda and pixels.dtype == torch.uint8
    host = pixels.cpu().numpy()
    for img, d in zip(imgs, descs):
        a = np.asarray(img if img.mode in ("RGB", "L") else img.convert("RGB"))
        a = a[:, :, None] if a.ndim == 2 else a
        assert (d.H, d.W, d.C, d.row_stride_bytes) == (a.shape[0], a.shape[1], a.shape[2], a.shape[1] * a.shape[2])
        assert np.array_equal(host[d.offset:d.offset + a.size], a.reshape(-1))
