from .decode_graph import DecodeRunner
from .generation import GenerationEngine
from .kv_cache import KVCacheFull, PagedKVCache
from .speculative import NgramProposer
from .llama import Llama, LlamaConfig, PRESETS as LLAMA_PRESETS, build_llama
from .quant import QuantLinear, quantize_weights_, weight_bytes
from .lora import AdapterSlotsFull, LoraAdapter, LoraLinear

__all__ = ["Llama", "LlamaConfig", "LLAMA_PRESETS", "build_llama", "PagedKVCache", "KVCacheFull", "GenerationEngine",
           "NgramProposer", "QuantLinear", "quantize_weights_", "weight_bytes", "LoraAdapter", "LoraLinear", "AdapterSlotsFull",
           "DecodeRunner"]
