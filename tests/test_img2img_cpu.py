"""Host logic of FLUX image-to-image, without a GPU: the truncated schedule (`get_timesteps`), the two new torch.ops schemas
(registered, no CPU kernel) and the new C-ABI entry points (exported, argument errors before any HIP call)."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")


@pytest.mark.parametrize("n,strength,steps", [(28, 0.6, 17), (28, 1.0, 28), (28, 0.01, 1), (28, 0.5, 14), (8, 0.6, 5),
                                              (8, 0.3, 3), (1, 1.0, 1), (50, 0.75, 38), (10, 0.95, 10), (28, 0.001, 1)])
def test_get_timesteps_table(n, strength, steps):
    from thinkdiff.models.flux_img2img import get_timesteps
    t_start = get_timesteps(n, strength)
    assert n - t_start == steps
    # diffusers' statement, restated
    init = min(n * strength, n)
    assert t_start == int(max(n - init, 0))


@pytest.mark.parametrize("n,strength", [(28, 0.0), (1, 0.0)])
def test_get_timesteps_without_a_step_is_refused(n, strength):
    from thinkdiff.models.flux_img2img import get_timesteps
    with pytest.raises(ValueError):
        get_timesteps(n, strength)


@pytest.mark.parametrize("strength", [-0.1, 1.01, 2.0])
def test_strength_outside_unit_interval_is_refused(strength):
    from thinkdiff.models.flux_img2img import get_timesteps
    with pytest.raises(ValueError, match="strength"):
        get_timesteps(28, strength)


def test_img2img_schemas_register_without_cpu_kernel():
    import thinkdiff.ops as ops
    for name in ("vae_encode_moments", "vae_latents_from_moments"):
        assert name in ops.SCHEMAS
        op = getattr(torch.ops.thinkdiff_hip, name)
        assert str(op.default._schema) == f"thinkdiff_hip::{name}{ops.SCHEMAS[name]}"
    mom = torch.zeros(16, 32, dtype=torch.bfloat16)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.thinkdiff_hip.vae_latents_from_moments(mom, None, None, 1.0, 0.3611, 0.1159, 4, 4)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.thinkdiff_hip.vae_encode_moments(1, torch.zeros(16, 16, 3, dtype=torch.uint8), 16, 16)


def test_encoder_entry_points_exported_and_refuse_bad_arguments():
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    for name in ("td_vae_enc_create", "td_vae_enc_destroy", "td_vae_enc_num_params", "td_vae_enc_param_info", "td_vae_enc_load_param",
                 "td_vae_enc_init_random", "td_vae_enc_output_shape", "td_vae_encode", "td_vae_latents_from_moments",
                 "td_vae_image_to_nhwc_bf16", "td_conv3x3_s2_nhwc_bf16"):
        assert hasattr(lib, name), name
    one = ctypes.c_void_p(256)                          # never dereferenced: the call must fail first
    assert lib.td_vae_enc_num_params(None) == 0
    assert lib.td_vae_enc_output_shape(None, 64, 64, None, None, None) == 2
    assert lib.td_vae_encode(None, one, 0, 64, 64, one, None) == 2
    rc = lib.td_conv3x3_s2_nhwc_bf16(one, one, one, one, 17, 16, 64, 64, None)
    assert rc == 2 and b"even" in lib.td_last_error()
    rc = lib.td_vae_latents_from_moments(one, None, None, ctypes.c_float(1.0), ctypes.c_float(1.0), ctypes.c_float(0.0), 16, 3, 4, one, None)
    assert rc == 2 and b"even" in lib.td_last_error()
    rc = lib.td_vae_image_to_nhwc_bf16(one, 7, 16, 16, one, 64, None)
    assert rc == 2 and b"format" in lib.td_last_error()
