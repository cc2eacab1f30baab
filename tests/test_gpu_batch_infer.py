"""Image-set inference (omnidata_amd/batch_infer.py, demo.py --batch_size): the files of a folder of images of different sizes
and modes, written by the batched pipeline, hold the pixels demo.py's per-image loop writes.  pytest -m gpu."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image, UnidentifiedImageError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("a", (400, 520, 3), "RGB"), ("b", (390, 384), "L"), ("c", (450, 420, 4), "RGBA"), ("d", (384, 384, 3), "RGB"),
          ("e", (700, 1000, 3), "RGB")]


def _folder(path):
    rng = np.random.default_rng(11)
    path.mkdir()
    for stem, shape, mode in SHAPES:
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8), mode).save(path / f"{stem}.png")
    return path


def _demo(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "demo.py")] + args, capture_output=True, text=True, env=env, cwd=ROOT,
                          timeout=600)


def _model(task, max_batch):
    from omnidata_amd.model import build_model
    return build_model(task, random_weights=0, max_batch=max_batch).to("cuda:0")


@pytest.mark.parametrize("task", ["normal", "depth"])
def test_batched_files_equal_the_per_image_loop(tmp_path, task):
    from omnidata_amd.batch_infer import BatchPredictor
    src = _folder(tmp_path / "in")
    r = _demo(["--task", task, "--img_path", str(src), "--output_path", str(tmp_path / "loop"), "--random-weights", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    files = glob.glob(str(src) + "/*")
    BatchPredictor(_model(task, 2), task, batch_size=2).predict_to_dir(files, str(tmp_path / "batch"))   # batches of 2, 2, 1
    names = sorted(os.listdir(tmp_path / "loop"))
    assert names == sorted(os.listdir(tmp_path / "batch")) and len(names) == 2 * len(SHAPES)
    for n in names:
        a, b = Image.open(tmp_path / "loop" / n), Image.open(tmp_path / "batch" / n)
        assert a.mode == b.mode and a.size == b.size, n
        assert np.array_equal(np.asarray(a), np.asarray(b)), n


def test_predict_yields_device_tensors_in_input_order(tmp_path):
    from omnidata_amd import preprocess as pp
    from omnidata_amd.batch_infer import BatchPredictor
    src = _folder(tmp_path / "in")
    files = sorted(glob.glob(str(src) + "/*"))
    model = _model("normal", 2)
    bp = BatchPredictor(model, "normal", batch_size=2, workers=64)
    assert bp.workers == 16
    outs = list(bp.predict(files[:2] + [Image.open(files[2]), np.asarray(Image.open(files[3]))] + files[4:]))
    assert len(outs) == len(files)
    for f, o in zip(files, outs):
        assert o.is_cuda and o.dtype == torch.uint8 and o.shape == (384, 384, 3)
        x = pp.image_to_input(Image.open(f), "normal").to("cuda:0")
        assert torch.equal(o, pp.normal_to_u8_gpu(model(x).clamp(0, 1)[0])), f    # this file's own result, not a neighbour's


def test_demo_cli_batch_size_prints_one_pair_of_lines_per_file_in_order(tmp_path):
    src = _folder(tmp_path / "in")
    out = tmp_path / "out"
    r = _demo(["--task", "normal", "--img_path", str(src), "--output_path", str(out), "--random-weights", "0", "--batch_size", "4"])
    assert r.returncode == 0, r.stderr[-2000:]
    files = glob.glob(str(src) + "/*")
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    lines = [l for l in r.stdout.splitlines() if l.startswith(("Reading input", "Writing output"))]
    want = []
    for f, s in zip(files, stems):
        want += [f"Reading input {f} ...", f"Writing output {os.path.join(str(out), s + '_normal.png')} ..."]
    assert lines == want
    for s in stems:
        assert Image.open(out / f"{s}_normal.png").size == (384, 384) and Image.open(out / f"{s}_rgb.png").size == (512, 512)


def test_unreadable_third_file_raises_after_the_first_two_are_written(tmp_path):
    from omnidata_amd.batch_infer import BatchPredictor
    src = _folder(tmp_path / "in")
    files = sorted(glob.glob(str(src) + "/*"))
    bad = src / "notes.txt"
    bad.write_text("not an image\n")
    order = files[:2] + [str(bad)] + files[2:]
    out = tmp_path / "out"
    with pytest.raises(UnidentifiedImageError):
        BatchPredictor(_model("normal", 4), "normal", batch_size=4).predict_to_dir(order, str(out))
    assert sorted(os.listdir(out)) == ["a_normal.png", "a_rgb.png", "b_normal.png", "b_rgb.png"]
    for s in ("a", "b"):
        assert Image.open(out / f"{s}_normal.png").size == (384, 384)
