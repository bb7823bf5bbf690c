"""cache_dtype -> KV pool dtype, where the plugin validates its config (no GPU)."""

import pytest
import torch

from vllm_neuron_amd._vllm_compat import FullAttentionSpec, SimpleCacheConfig
from vllm_neuron_amd.worker.mi355x_model_loader import resolve_kv_cache_dtype


def test_kv_cache_dtype_mapping():
    assert SimpleCacheConfig().cache_dtype == "auto"
    assert resolve_kv_cache_dtype("auto", {}) == resolve_kv_cache_dtype("bfloat16", {}) == "bfloat16"
    assert resolve_kv_cache_dtype("fp8", {}) == resolve_kv_cache_dtype("fp8_e4m3", {}) == "fp8_e4m3"
    assert resolve_kv_cache_dtype("auto", {"kv_cache_quant": True}) == "fp8_e4m3"
    with pytest.raises(ValueError):
        resolve_kv_cache_dtype("fp8_e5m2", {})
    spec = {dt: FullAttentionSpec(block_size=32, num_kv_heads=2, head_size=64, dtype=dt, sliding_window=None)
            for dt in (torch.bfloat16, torch.float8_e4m3fn)}
    assert spec[torch.float8_e4m3fn].page_size_bytes * 2 == spec[torch.bfloat16].page_size_bytes
