"""Shared by the image-resize tests: the shape / filter / content lists, td_resize_coeffs through ctypes, and a numpy restatement of the
integer rule the kernels implement (horizontal pass, uint8 intermediate, vertical pass; int32 accumulation from 1 << 21, clip8(acc >> 22)).
The reference of every test is Pillow's own `Image.resize`; this restatement only shows, without a GPU, that the host tables plus that
rule give Pillow's bytes."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")

LANCZOS, BILINEAR, BICUBIC = 1, 2, 3
FILTERS = {"lanczos": LANCZOS, "bilinear": BILINEAR, "bicubic": BICUBIC}

# (in_h, in_w, out_h, out_w): the smallest shapes at which each thing can go wrong
SHAPES = [
    (37, 53, 16, 16),        # both axes down
    (16, 24, 48, 40),        # both axes up
    (64, 64, 64, 32),        # horizontal pass only
    (64, 64, 32, 64),        # vertical pass only
    (64, 64, 64, 64),        # no pass
    (9, 200, 27, 31),        # one axis up, one down
    (113, 77, 112, 84),      # scale near 1
    (1, 1, 5, 7),            # window clipped at both ends
    (5, 7, 1, 1),            # window clipped at both ends
    (600, 450, 28, 28),      # ksize 131 (lanczos)
]
SHAPE_IDS = [f"{a}x{b}to{c}x{d}" for a, b, c, d in SHAPES]
CONTENTS = ["noise", "checker1", "checker3"]
# in_c -> out_c forms of td_image_resize_u8, each on two shapes
CHANNEL_FORMS = [(3, 3), (1, 1), (1, 3), (4, 3)]
CHANNEL_SHAPES = [(37, 53, 16, 16), (16, 24, 48, 40)]


def content(kind, h, w, c, seed=0):
    """uint8 [h, w, c]: seeded uniform noise, or a 0 / 255 checkerboard of the given period (it sends bicubic and lanczos past both ends of clip8)."""
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)
    period = int(kind[len("checker"):])
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy // period) + (xx // period)) % 2 * 255).astype(np.uint8)
    out = np.repeat(board[:, :, None], c, axis=2)
    if c > 1:
        out[:, :, 1] = 255 - out[:, :, 1]          # channels differ, so a channel mix-up shows
    return np.ascontiguousarray(out)


def pil_resize(arr, out_h, out_w, resample, out_c=None):
    """Pillow on the same array: mode from the channel count, convert("RGB") first when the channel count changes."""
    from PIL import Image
    h, w, c = arr.shape
    im = Image.fromarray(arr[:, :, 0] if c == 1 else arr, mode={1: "L", 3: "RGB", 4: "RGBA"}[c])
    if out_c is not None and out_c != c:
        assert out_c == 3
        im = im.convert("RGB")
    got = np.asarray(im.resize((out_w, out_h), resample=resample), dtype=np.uint8)
    return got[:, :, None] if got.ndim == 2 else got


def load_lib():
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    lib.td_resize_coeffs.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    lib.td_resize_coeffs.restype = ctypes.c_int
    return lib


def coeffs(lib, in_size, out_size, resample):
    """(bounds int32 [out, 2], kk int32 [out, ksize]) from td_resize_coeffs: the query form first, then the fill."""
    ks = ctypes.c_int(-1)
    rc = lib.td_resize_coeffs(in_size, out_size, resample, None, None, ctypes.byref(ks))
    assert rc == 0, lib.td_last_error()
    ksize = ks.value
    bounds = np.full((out_size, 2), -7, dtype=np.int32)
    kk = np.full((out_size, ksize), -7, dtype=np.int32)
    ks2 = ctypes.c_int(-1)
    rc = lib.td_resize_coeffs(in_size, out_size, resample, bounds.ctypes.data, kk.ctypes.data, ctypes.byref(ks2))
    assert rc == 0 and ks2.value == ksize, lib.td_last_error()
    return bounds, kk


def _pass(src, bounds, kk):
    """One pass along axis 0 of src uint8 [n_in, ...] -> uint8 [n_out, ...] by the integer rule."""
    out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
    s = src.astype(np.int32)
    for o in range(bounds.shape[0]):
        lo, cnt = int(bounds[o, 0]), int(bounds[o, 1])
        acc = np.full(src.shape[1:], 1 << 21, dtype=np.int32)
        for i in range(cnt):
            acc += s[lo + i] * kk[o, i]
        out[o] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return out


def resize_restated(lib, arr, out_h, out_w, resample):
    """arr uint8 [h, w, c] -> uint8 [out_h, out_w, c]: horizontal pass, then vertical; a pass whose size does not change is skipped."""
    h, w, _ = arr.shape
    x = arr
    if out_w != w:
        b, k = coeffs(lib, w, out_w, resample)
        x = np.ascontiguousarray(_pass(np.ascontiguousarray(x.transpose(1, 0, 2)), b, k).transpose(1, 0, 2))
    if out_h != h:
        b, k = coeffs(lib, h, out_h, resample)
        x = _pass(x, b, k)
    return x
