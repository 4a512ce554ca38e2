"""td_image_resize_u8 on the GPU against Pillow's `Image.resize` on the same array: equality, not a tolerance (after the host-made coefficient
tables the resampler is integer arithmetic).  Shapes, filters and contents come from image_resize_common; the destination lies inside a larger
buffer whose guard bytes on both sides must survive; `_hip.image_resize_u8` and `torch.ops.thinkdiff_hip.image_resize_u8` give the same bytes."""
import numpy as np
import pytest
import torch

import image_resize_common as C

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTES = 0xA5, 257        # an odd offset: the destination is not even 2-byte aligned


@pytest.fixture(scope="module", autouse=True)
def _op_layer():
    from thinkdiff import ops          # loads lib/libthinkdiff_torch_ops.so: torch.ops.thinkdiff_hip.*
    return ops.register()


def _resize_guarded(hip, src, out_h, out_w, resample, out_c):
    """-> (result [out_h, out_w, out_c] on the host, guards untouched?)"""
    n = out_h * out_w * out_c
    buf = torch.full((n + 2 * GUARD_BYTES,), GUARD, dtype=torch.uint8, device="cuda")
    out = buf[GUARD_BYTES:GUARD_BYTES + n].view(out_h, out_w, out_c)
    got = hip.image_resize_u8(src, out_h, out_w, resample, out_channels=out_c, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu()
    intact = bool((host[:GUARD_BYTES] == GUARD).all()) and bool((host[GUARD_BYTES + n:] == GUARD).all())
    return host[GUARD_BYTES:GUARD_BYTES + n].view(out_h, out_w, out_c), intact


@pytest.mark.parametrize("fname", list(C.FILTERS))
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.SHAPE_IDS)
def test_resize_equals_pillow(hip, shape, fname):
    in_h, in_w, out_h, out_w = shape
    f = C.FILTERS[fname]
    for kind in C.CONTENTS:
        arr = C.content(kind, in_h, in_w, 3, seed=in_h * 1000 + in_w)
        want = torch.from_numpy(C.pil_resize(arr, out_h, out_w, f).copy())
        src = torch.from_numpy(arr).cuda()
        got, intact = _resize_guarded(hip, src, out_h, out_w, f, 3)
        assert intact, (shape, fname, kind, "bytes outside the destination were written")
        assert torch.equal(got, want), (shape, fname, kind, int((got.int() - want.int()).abs().max()), int((got != want).sum()))
        op = torch.ops.thinkdiff_hip.image_resize_u8(src, out_h, out_w, f, None)
        assert op.shape == want.shape and op.dtype == torch.uint8 and torch.equal(op.cpu(), want), (shape, fname, kind, "torch op")


def test_checkerboards_reach_both_ends_of_clip8():
    """What the checkerboard contents are for: before clipping, bicubic and lanczos leave [0, 255] on both sides."""
    lib = C.load_lib()
    arr = C.content("checker3", 16, 24, 3)
    for f in (C.BICUBIC, C.LANCZOS):
        b, k = C.coeffs(lib, 24, 40, f)
        row = arr[0, :, 0].astype(np.int64)
        acc = np.array([(1 << 21) + sum(int(row[b[o, 0] + i]) * int(k[o, i]) for i in range(b[o, 1])) for o in range(40)])
        assert (acc >> 22).min() < 0 and (acc >> 22).max() > 255


@pytest.mark.parametrize("form", C.CHANNEL_FORMS, ids=[f"{a}to{b}" for a, b in C.CHANNEL_FORMS])
@pytest.mark.parametrize("shape", C.CHANNEL_SHAPES, ids=[f"{a}x{b}to{c}x{d}" for a, b, c, d in C.CHANNEL_SHAPES])
def test_channel_forms_equal_pillow_convert_rgb(hip, shape, form):
    in_h, in_w, out_h, out_w = shape
    in_c, out_c = form
    for f in C.FILTERS.values():
        for kind in ("noise", "checker1"):
            arr = C.content(kind, in_h, in_w, in_c, seed=7 + in_c)
            want = torch.from_numpy(C.pil_resize(arr, out_h, out_w, f, out_c=out_c).copy())
            src = torch.from_numpy(arr).cuda()
            got, intact = _resize_guarded(hip, src, out_h, out_w, f, out_c)
            assert intact and got.shape == want.shape and torch.equal(got, want), (shape, form, f, kind)
            op = torch.ops.thinkdiff_hip.image_resize_u8(src, out_h, out_w, f, out_c)
            assert torch.equal(op.cpu(), want), (shape, form, f, kind, "torch op")
    # one pass only, and no pass at all (the channel conversion alone), for the forms that change the channel count
    if in_c != out_c:
        arr = C.content("noise", in_h, in_w, in_c, seed=3)
        for oh, ow in ((in_h, out_w), (out_h, in_w), (in_h, in_w)):
            want = torch.from_numpy(C.pil_resize(arr, oh, ow, C.BICUBIC, out_c=out_c).copy())
            got, intact = _resize_guarded(hip, torch.from_numpy(arr).cuda(), oh, ow, C.BICUBIC, out_c)
            assert intact and torch.equal(got, want), (shape, form, oh, ow)


def test_binding_forms_and_refusals(hip):
    arr = C.content("noise", 37, 53, 1, seed=1)
    want = torch.from_numpy(C.pil_resize(arr, 16, 16, C.LANCZOS).copy())
    a = hip.image_resize_u8(torch.from_numpy(arr[:, :, 0].copy()).cuda(), 16, 16, C.LANCZOS)          # a 2-D image is one channel
    assert a.shape == (16, 16, 1) and torch.equal(a.cpu(), want)
    src = torch.from_numpy(C.content("noise", 8, 8, 3)).cuda()
    with pytest.raises(hip.ThinkDiffHipError, match="HAMMING"):
        hip.image_resize_u8(src, 4, 4, 5)
    with pytest.raises(hip.ThinkDiffHipError, match="in_c=3 -> out_c=1"):
        hip.image_resize_u8(src, 4, 4, C.BICUBIC, out_channels=1)
    with pytest.raises(RuntimeError, match="NEAREST"):
        torch.ops.thinkdiff_hip.image_resize_u8(src, 4, 4, 0, None)
    with pytest.raises(RuntimeError, match="must be 1"):
        torch.ops.thinkdiff_hip.image_resize_u8(src, 0, 4, C.BICUBIC, None)
    with pytest.raises(RuntimeError, match="contiguous uint8"):
        torch.ops.thinkdiff_hip.image_resize_u8(src.float(), 4, 4, C.BICUBIC, None)
    # the lookup that follows the resize in the processors: out[c, y, x] = lut[c, img[y, x, c]]
    lut = torch.randn(3, 256)
    img = torch.from_numpy(C.content("noise", 9, 11, 3, seed=2))
    got = hip.image_lut_chw_f32(img.cuda(), lut.cuda())
    want = torch.stack([lut[c][img[:, :, c].long()] for c in range(3)])
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)
