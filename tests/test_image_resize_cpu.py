"""PIL-exact image resize, the parts that need no GPU: td_resize_coeffs' tables applied by the integer rule in numpy equal Pillow's
`Image.resize` byte for byte, and every refusal of td_resize_coeffs / td_image_resize_u8 comes back as TD_ERR_INVALID with a message that
names the value, before any HIP call."""
import ctypes

import numpy as np
import pytest

import image_resize_common as C


@pytest.fixture(scope="module")
def lib():
    return C.load_lib()


@pytest.mark.parametrize("fname", list(C.FILTERS))
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.SHAPE_IDS)
def test_tables_with_the_integer_rule_equal_pillow(lib, shape, fname):
    in_h, in_w, out_h, out_w = shape
    f = C.FILTERS[fname]
    for kind in C.CONTENTS:
        arr = C.content(kind, in_h, in_w, 3, seed=in_h * 1000 + in_w)
        got = C.resize_restated(lib, arr, out_h, out_w, f)
        want = C.pil_resize(arr, out_h, out_w, f)
        assert got.shape == want.shape and np.array_equal(got, want), (shape, fname, kind, int(np.abs(got.astype(int) - want.astype(int)).max()))


def test_one_channel_image_equals_pillow(lib):
    arr = C.content("noise", 90, 130, 1, seed=5)
    for f in C.FILTERS.values():
        assert np.array_equal(C.resize_restated(lib, arr, 56, 84, f), C.pil_resize(arr, 56, 84, f))


def test_table_layout(lib):
    """ksize = ceil(support * max(in / out, 1)) * 2 + 1; rows zero past count; windows inside the source; weights sum to 2^22 up to rounding."""
    for (n_in, n_out, f, ksize) in [(600, 28, C.LANCZOS, 131), (450, 28, C.LANCZOS, 99), (16, 48, C.BICUBIC, 5), (16, 48, C.BILINEAR, 3), (53, 16, C.BICUBIC, 15)]:
        b, k = C.coeffs(lib, n_in, n_out, f)
        assert k.shape == (n_out, ksize)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= ksize).all()
        for o in range(n_out):
            assert not k[o, b[o, 1]:].any()
            assert abs(int(k[o].sum()) - (1 << 22)) <= ksize      # each weight is rounded to 2^-22 on its own
    # the query form writes ksize only and agrees with the fill
    ks = ctypes.c_int(0)
    assert lib.td_resize_coeffs(600, 28, C.LANCZOS, None, None, ctypes.byref(ks)) == 0 and ks.value == 131


def test_python_binding_caches_tables_per_axis():
    from thinkdiff import _hip
    assert hasattr(_hip.lib(), "td_resize_coeffs") and hasattr(_hip.lib(), "td_image_resize_u8")
    tab, ksize = _hip.resize_coeffs(600, 28, 1)
    assert ksize == 131 and tab.dtype == np.int32 and tab.shape == (2 * 28 + 28 * 131,) and not tab.flags.writeable
    assert _hip.resize_coeffs(600, 28, 1)[0] is tab
    b, k = C.coeffs(C.load_lib(), 600, 28, 1)
    assert np.array_equal(tab[:56].reshape(28, 2), b) and np.array_equal(tab[56:].reshape(28, 131), k)
    with pytest.raises(_hip.ThinkDiffHipError, match="BOX"):
        _hip.resize_coeffs(8, 4, 4)


def test_the_op_layer_registers_the_resize():
    import torch
    from thinkdiff import ops
    assert str(torch.ops.thinkdiff_hip.image_resize_u8.default._schema) == "thinkdiff_hip::image_resize_u8" + ops.SCHEMAS["image_resize_u8"]


def test_coeff_refusals(lib):
    ks = ctypes.c_int(0)
    buf = (ctypes.c_int * 64)()
    cases = [
        ("in_size", lambda: lib.td_resize_coeffs(0, 4, 3, None, None, ctypes.byref(ks)), b"in_size=0"),
        ("in_size<0", lambda: lib.td_resize_coeffs(-5, 4, 3, None, None, ctypes.byref(ks)), b"in_size=-5"),
        ("out_size", lambda: lib.td_resize_coeffs(4, 0, 3, None, None, ctypes.byref(ks)), b"out_size=0"),
        ("out_size<0", lambda: lib.td_resize_coeffs(4, -2, 3, None, None, ctypes.byref(ks)), b"out_size=-2"),
        ("nearest", lambda: lib.td_resize_coeffs(4, 4, 0, None, None, ctypes.byref(ks)), b"NEAREST"),
        ("box", lambda: lib.td_resize_coeffs(4, 4, 4, None, None, ctypes.byref(ks)), b"BOX"),
        ("hamming", lambda: lib.td_resize_coeffs(4, 4, 5, None, None, ctypes.byref(ks)), b"HAMMING"),
        ("unknown", lambda: lib.td_resize_coeffs(4, 4, 9, None, None, ctypes.byref(ks)), b"filter=9"),
        ("one buffer", lambda: lib.td_resize_coeffs(4, 4, 3, ctypes.addressof(buf), None, ctypes.byref(ks)), b"both"),
        ("no ksize", lambda: lib.td_resize_coeffs(4, 4, 3, None, None, None), b"ksize"),
        ("window", lambda: lib.td_resize_coeffs(2 ** 31 - 1, 1, 1, None, None, ctypes.byref(ks)), b"in_size=2147483647"),
    ]
    for what, call, needle in cases:
        rc = call()
        msg = lib.td_last_error()
        assert rc == 2, (what, rc, msg)
        assert needle in msg and b"td_resize_coeffs" in msg, (what, msg)


def test_launch_refusals_come_before_any_launch(lib):
    """td_image_resize_u8 on a machine without a GPU: each of these must return before it touches a pointer or the HIP runtime."""
    one = ctypes.c_void_p(256)                          # never dereferenced

    def call(in_h=8, in_w=8, in_c=3, out_h=4, out_w=4, out_c=3, hb=one, hk=one, kh=5, vb=one, vk=one, kv=5, tmp=one, src=one, dst=one):
        return lib.td_image_resize_u8(src, in_h, in_w, in_c, dst, out_h, out_w, out_c, hb, hk, kh, vb, vk, kv, tmp, None)

    cases = [
        ("in_h", lambda: call(in_h=0), b"in_h=0"),
        ("in_w", lambda: call(in_w=-3), b"in_w=-3"),
        ("out_h", lambda: call(out_h=0), b"out_h=0"),
        ("out_w", lambda: call(out_w=-1), b"out_w=-1"),
        ("3->1", lambda: call(in_c=3, out_c=1), b"in_c=3 -> out_c=1"),
        ("2->2", lambda: call(in_c=2, out_c=2), b"in_c=2 -> out_c=2"),
        ("4->4", lambda: call(in_c=4, out_c=4), b"in_c=4 -> out_c=4"),
        ("3->4", lambda: call(in_c=3, out_c=4), b"in_c=3 -> out_c=4"),
        ("no horizontal table", lambda: call(hb=None), b"in_w=8 -> out_w=4"),
        ("no horizontal weights", lambda: call(hk=None), b"in_w=8 -> out_w=4"),
        ("horizontal ksize", lambda: call(kh=0), b"ksize=0"),
        ("no vertical table", lambda: call(vb=None, vk=None), b"in_h=8 -> out_h=4"),
        ("vertical ksize", lambda: call(kv=-1), b"ksize=-1"),
        ("no tmp", lambda: call(tmp=None), b"tmp"),
        ("null src", lambda: call(src=None), b"src"),
        ("oversize destination", lambda: call(in_h=1, in_w=1, out_h=65536, out_w=65536), b"32-bit index"),
        ("oversize source", lambda: call(in_h=40000, in_w=40000), b"32-bit index"),
        ("oversize intermediate", lambda: call(in_h=2 ** 30, in_w=1, in_c=1, out_c=1, out_h=1, out_w=4), b"32-bit index"),
    ]
    for what, c, needle in cases:
        rc = c()
        msg = lib.td_last_error()
        assert rc == 2, (what, rc, msg)
        assert needle in msg and b"td_image_resize_u8" in msg, (what, msg)
    # the table lookup that follows the resize in the processors
    assert lib.td_image_lut_chw_f32(one, 0, 4, 3, one, one, None) == 2 and b"H=0" in lib.td_last_error()
    assert lib.td_image_lut_chw_f32(one, 4, 4, 5, one, one, None) == 2 and b"C=5" in lib.td_last_error()
