"""Model registry (reference thinkdiff/models/__init__.py): importing this package registers the archs."""
from ..common.registry import registry
from .base_model import BaseModel
from .blip_vision_t5_decoder import BlipVisionT5DecoderForConditionalGeneration, build_vision_projector
from .flux_control import FluxControlPipelineRewritePrompt
from .flux_controlnet import FluxControlNetConfig, FluxControlNetModel, FluxControlNetPipelineRewritePrompt, FluxMultiControlNetModel
from .flux_fill import FluxFillPipelineRewritePrompt
from .flux_img2img import FluxImg2ImgPipelineRewritePrompt
from .flux_inpaint import FluxInpaintPipelineRewritePrompt
from .flux_kontext import FluxKontextPipelineRewritePrompt
from .flux_prompt import FluxPipelineRewritePrompt
from .flux_redux import FluxPriorReduxPipelineRewritePrompt, ReduxImageEncoder
from .flux_transformer import FirstBlockCacheConfig, FluxTransformer2DModel, FluxTransformerConfig, apply_first_block_cache
from .mllama_vllm_t5_embed_decoder_2 import MllamaVllmT5EmbedDecoderForConditionalGeneration_5
from .mllama_vllm_generate_1 import MllamaVllmGenerate_1
from .qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine, SamplingParams

__all__ = ["registry", "BaseModel", "BlipVisionT5DecoderForConditionalGeneration", "build_vision_projector",
           "FluxPipelineRewritePrompt", "FluxImg2ImgPipelineRewritePrompt", "FluxInpaintPipelineRewritePrompt",
           "FluxFillPipelineRewritePrompt", "FluxControlPipelineRewritePrompt", "FluxKontextPipelineRewritePrompt",
           "FluxControlNetPipelineRewritePrompt", "FluxControlNetModel", "FluxControlNetConfig", "FluxMultiControlNetModel",
           "FluxTransformer2DModel", "FluxTransformerConfig", "FirstBlockCacheConfig", "apply_first_block_cache",
           "FluxPriorReduxPipelineRewritePrompt", "ReduxImageEncoder"]
