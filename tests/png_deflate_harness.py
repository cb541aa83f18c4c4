"""What the GPU tests of the three deflate paths share (tests/test_gpu_png_deflate.py, test_gpu_png_huffman.py, test_gpu_png16_deflate.py): a
frame through the entry point into a guarded result buffer, the reference's result computed once per key, and the comparison -- header and
stream byte for byte, then the stream inflated with zlib.  A path is described by a Format."""
import zlib
from typing import Any, Callable, NamedTuple

import numpy as np
import pytest

from tests.yuv_harness import GUARD, _once

FIXED, DYNAMIC = 0, 1


class Format(NamedTuple):
    tag: str           # the name space of the cached references
    ref: Any           # the reference module: HEADER_BYTES, result_bytes, band_rows, inflate
    pixel: int         # bytes of a pixel on the card
    sizes: str         # pa.<sizes>(w, h): the result buffer's bytes
    band_rows: str     # pa.<band_rows>(w)
    deflate: str       # pa.<deflate>(frame_ptr, out_ptr, w, h, stream=, timed=, codes=)
    codes: int         # the codes a test means that names none
    stage: Callable    # the frame as a numpy array -> the contiguous bytes that go to the card
    encode: Callable   # the frame -> ({fixed: the result buffer up to the end of the stream}, the bands' details or None, the raw scanlines)


def _deflate(fmt, pa, frame, codes=None, buf=None, timed=False, stream=0):
    """The frame (a numpy array, or a tensor that is on the card already) through the entry point -> the whole result buffer as host bytes; the
    64 guard bytes behind it must survive."""
    import torch

    h, w = frame.shape[:2]
    nbytes = getattr(pa, fmt.sizes)(w, h)
    assert nbytes == fmt.ref.result_bytes(w, h) and getattr(pa, fmt.band_rows)(w) == fmt.ref.band_rows(w)
    staged = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(fmt.stage(frame)).cuda()
    if buf is None:
        buf = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert buf.numel() == nbytes + 64 and buf.data_ptr() % 16 == 0 and staged.data_ptr() % 16 == 0 and staged.numel() * staged.element_size() == fmt.pixel * w * h
    ms = getattr(pa, fmt.deflate)(staged.data_ptr(), buf.data_ptr(), w, h, stream=stream or torch.cuda.current_stream().cuda_stream, timed=timed,
                                  codes=fmt.codes if codes is None else codes)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[nbytes:] == GUARD).all(), "written behind the result buffer"
    return (host[:nbytes].tobytes(), ms) if timed else host[:nbytes].tobytes()


def _reference(fmt, key, frame, fixed=False):
    """(result buffer up to the end of the stream, the bands' details, the raw scanlines), computed once per key."""
    results, bands, raw = _once((fmt.tag, key), lambda: fmt.encode(frame))
    return results[fixed], bands, raw


def _assert_matches(fmt, got, frame, what, key=None, fixed=None):
    """Header and stream against the reference, byte for byte; the stream inflates to the raw scanlines.  Returns the bands' details."""
    frame = frame if isinstance(frame, np.ndarray) else frame.cpu().numpy()
    key = key or (what, frame.shape, zlib.crc32(np.ascontiguousarray(frame)))  # (a name alone may be used for two frames)
    want, bands, raw = _reference(fmt, key, frame, fmt.codes == FIXED if fixed is None else fixed)
    n = int(np.frombuffer(got[12:16], "<u4")[0])
    if got[: fmt.ref.HEADER_BYTES + n] != want:
        g, r = np.frombuffer(got[: len(want)], np.uint8), np.frombuffer(want, np.uint8)
        chosen = f" (bands choose {[b['dynamic'] for b in bands][:8]})" if bands else ""
        assert got[:64] == want[:64], f"{what}: header {np.frombuffer(got[:28], '<u4').tolist()}, want {np.frombuffer(want[:28], '<u4').tolist()}{chosen}"
        first = int(np.flatnonzero(g != r)[0])
        pytest.fail(f"{what}: {int((g != r).sum())} of {len(want)} bytes differ, the first at {first} (stream byte {first - 64}): got {g[first: first + 8].tolist()}, want {r[first: first + 8].tolist()}")
    assert fmt.ref.inflate(got) == raw, what
    return bands


def _check(fmt, pa, frame, what, codes=None):
    return _assert_matches(fmt, _deflate(fmt, pa, frame, codes=codes), frame, what, fixed=(fmt.codes if codes is None else codes) == FIXED)
