from .generation import GenerationEngine
from .kv_cache import KVCacheFull, PagedKVCache
from .speculative import NgramProposer
from .llama import Llama, LlamaConfig, PRESETS as LLAMA_PRESETS, build_llama

__all__ = ["Llama", "LlamaConfig", "LLAMA_PRESETS", "build_llama", "PagedKVCache", "KVCacheFull", "GenerationEngine",
           "NgramProposer"]
