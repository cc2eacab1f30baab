"""The look-ahead decode of omnidata_amd/batch_infer.py as a free function: order, what is queued when a chunk is handed out, and
the crop path's rule for a file that does not decode.  No GPU, no library."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
from PIL import Image, UnidentifiedImageError

from omnidata_amd import batch_infer
from omnidata_amd.batch_infer import lookahead


def _items(n):
    """PIL images and arrays in turn, told apart by their widths."""
    rng = np.random.default_rng(3)
    arrays = [rng.integers(0, 256, (4, 5 + i, 3), dtype=np.uint8) for i in range(n)]
    return [Image.fromarray(a) if i % 2 == 0 else a for i, a in enumerate(arrays)]


def _width(item):
    return item.size[0] if isinstance(item, Image.Image) else item.shape[1]


@pytest.fixture
def recorded(monkeypatch):
    """-> (submitted, decoded, Pool): a wrapper stands behind batch_infer._decode and notes every item it decodes; Pool is a
    ThreadPoolExecutor that notes every item handed to submit() with that wrapper, at the moment of the call."""
    submitted, decoded, decode = [], [], batch_infer._decode

    def wrapper(item):
        decoded.append(item)
        return decode(item)

    class Pool(ThreadPoolExecutor):
        def submit(self, fn, item):
            assert fn is wrapper
            submitted.append(item)
            return super().submit(fn, item)

    monkeypatch.setattr(batch_infer, "_decode", wrapper)
    return submitted, decoded, Pool


def test_chunks_come_out_in_order_and_the_next_one_is_queued_first(recorded):
    record, _, Pool = recorded
    items = _items(7)
    chunks = [[0, 1, 2], [5, 6], [3, 4]]                                        # any index lists, as plan_full_frame buckets them
    seen = []
    with Pool(2) as pool:
        for k, (idxs, images, error) in enumerate(lookahead(pool, items, chunks)):
            assert error is None and idxs == chunks[k]
            assert [_width(im) for im in images] == [5 + i for i in idxs]       # the decoded items of this chunk, in its order
            queued = sum(len(c) for c in chunks[:k + 2])                         # this chunk and the next, nothing further
            assert len(record) == queued and [_width(it) for it in record] == [5 + i for c in chunks[:k + 2] for i in c]
            seen.append(idxs)
    assert seen == chunks and len(record) == 7


@pytest.mark.parametrize("j", [0, 1, 2])
def test_stop_on_error_hands_out_the_images_before_the_failure_and_ends(tmp_path, recorded, j):
    submitted, decoded, Pool = recorded
    bad = tmp_path / "notes.txt"
    bad.write_text("not an image\n")
    items = _items(12)
    items[3 + j] = str(bad)                                                      # position j of the second chunk
    chunks = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]]
    got = []
    with Pool(2) as pool:
        for idxs, images, error in lookahead(pool, items, chunks, stop_on_error=True):
            got.append((idxs, [_width(im) for im in images], error))
    assert len(got) == 2 and got[0][:2] == ([0, 1, 2], [5, 6, 7]) and got[0][2] is None
    idxs, widths, error = got[1]
    assert idxs == [3, 4, 5] and widths == [8 + i for i in range(j)] and isinstance(error, UnidentifiedImageError)
    # the third chunk was queued behind the failing one (the look-ahead) and cancelled where it had not started; the fourth never
    assert len(submitted) == 9 and all(it is not items[i] for it in decoded for i in chunks[3])


def test_without_stop_on_error_the_exception_propagates(tmp_path):
    bad = tmp_path / "notes.txt"
    bad.write_text("not an image\n")
    items = _items(4)
    items[2] = str(bad)
    with ThreadPoolExecutor(2) as pool:
        gen = lookahead(pool, items, [[0, 1], [2, 3]])
        assert next(gen)[0] == [0, 1]
        with pytest.raises(UnidentifiedImageError):
            next(gen)


def test_an_empty_input_yields_nothing():
    with ThreadPoolExecutor(2) as pool:
        assert list(lookahead(pool, [], [])) == []
        assert list(lookahead(pool, [], [], stop_on_error=True)) == []
