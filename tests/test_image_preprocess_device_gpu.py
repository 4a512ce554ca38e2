"""The users of td_image_resize_u8: QwenChatFrontend._preprocess_on_device with PIL's own resize made to raise (so the host resize is provably
gone from that path) against transformers' processor computed beforehand, and the two stand-in processors with `device=` against their own
host path -- equality everywhere."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _images():
    from PIL import Image
    rng = np.random.default_rng(11)
    return {
        "RGB": [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in [(75, 100), (28, 30), (140, 84)]],
        "L": [Image.fromarray(rng.integers(0, 256, (90, 130), dtype=np.uint8), mode="L")],
        "RGBA": [Image.fromarray(rng.integers(0, 256, (64, 200, 4), dtype=np.uint8), mode="RGBA")],
    }


def test_qwen2_preprocessing_runs_without_the_host_resize(hip, monkeypatch):
    from PIL import Image
    from transformers import Qwen2VLImageProcessor
    from thinkdiff.models.qwen2_vl import QwenChatFrontend
    from thinkdiff.models.vision_towers import HipQwen2VisionTransformer

    class Front(QwenChatFrontend):
        pass
    f = Front()
    f.visual = HipQwen2VisionTransformer.from_random(embed_dim=320, depth=1, num_heads=4, mlp_ratio=2, out_hidden=256, seed=1)
    f.image_processor = Qwen2VLImageProcessor(min_pixels=56 * 56, max_pixels=28 * 28 * 40)
    assert type(f.image_processor).__name__ == "Qwen2VLImageProcessorPil"
    sets = _images()
    sets["mixed"] = sets["RGB"] + sets["L"] + sets["RGBA"]                 # more than two images: the threaded host stage
    want = {mode: f.image_processor(images=imgs, return_tensors="pt") for mode, imgs in sets.items()}   # the reference, with PIL's resize intact

    def refuse(self, *a, **k):
        raise AssertionError("PIL.Image.Image.resize was called: the resize is meant to run on the device")
    monkeypatch.setattr(Image.Image, "resize", refuse)
    with pytest.raises(AssertionError, match="meant to run on the device"):
        sets["RGB"][0].resize((8, 8))
    for mode, imgs in sets.items():
        got = f._preprocess_on_device(imgs)
        assert got is not None, mode
        assert got["image_grid_thw"] == want[mode]["image_grid_thw"].tolist(), mode
        K = want[mode]["pixel_values"].shape[1]
        pv = got["pixel_values"].cpu()
        assert pv.shape == (want[mode]["pixel_values"].shape[0], f.visual.padded_patch_dim) and pv.dtype == torch.bfloat16, mode
        assert torch.equal(pv[:, :K], want[mode]["pixel_values"].bfloat16()) and torch.count_nonzero(pv[:, K:]) == 0, mode


@pytest.mark.parametrize("size", [(375, 500), (60, 45)], ids=["375x500", "60x45"])
def test_redux_processor_on_device_equals_its_host_path(hip, size):
    from PIL import Image
    from thinkdiff.models.flux_redux import ReduxDefaultImageProcessor
    rng = np.random.default_rng(size[0])
    imgs = [Image.fromarray(rng.integers(0, 256, (*size, 3), dtype=np.uint8)), Image.fromarray(rng.integers(0, 256, size, dtype=np.uint8), mode="L"),
            Image.fromarray(rng.integers(0, 256, (*size, 4), dtype=np.uint8), mode="RGBA")]
    want = ReduxDefaultImageProcessor(size=84).preprocess(images=imgs).pixel_values
    got = ReduxDefaultImageProcessor(size=84, device="cuda")(imgs).pixel_values
    assert got.is_cuda and got.dtype == want.dtype == torch.float32 and got.shape == want.shape == (3, 3, 84, 84)
    assert torch.equal(got.cpu(), want)
    one = ReduxDefaultImageProcessor(size=84, image_mean=0.4, image_std=0.3, device="cuda")(imgs[0]).pixel_values
    assert torch.equal(one.cpu(), ReduxDefaultImageProcessor(size=84, image_mean=0.4, image_std=0.3)(imgs[0]).pixel_values)


@pytest.mark.parametrize("size", [(375, 500), (100, 224)], ids=["375x500", "100x224"])
def test_blip_stand_in_processor_on_device_equals_its_host_path(hip, size):
    from PIL import Image
    from thinkdiff.models.providers import SyntheticImageProcessor
    rng = np.random.default_rng(size[1])
    host, dev = SyntheticImageProcessor(), SyntheticImageProcessor(device="cuda")
    for im in (Image.fromarray(rng.integers(0, 256, (*size, 3), dtype=np.uint8)), Image.fromarray(rng.integers(0, 256, size, dtype=np.uint8), mode="L")):
        want = host(im)["pixel_values"]
        got = dev(im)["pixel_values"]
        assert got.is_cuda and got.dtype == want.dtype == torch.float32 and got.shape == want.shape == (1, 3, 224, 224)
        assert torch.equal(got.cpu(), want)
