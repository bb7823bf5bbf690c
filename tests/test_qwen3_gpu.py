"""Qwen3 (per-head QK-norm) end to end against the committed HF-transformers golden (tools/gen_qwen3_golden.py)."""

import json
import os
from types import SimpleNamespace

import pytest
import torch
from safetensors import safe_open

from oracle.paged_decoder import DecoderConfig
from oracle.synth import make_prompts, make_weights, weights_checksum
from tests.helpers import decode_inputs, prefill_inputs

GOLD = os.path.join(os.path.dirname(__file__), "golden", "hf_qwen3_golden.safetensors")


def golden():   # -> (config, weights incl. the q_norm / k_norm gains, greedy ids [4][12], fp32 logits [4][12, V])
    f = safe_open(GOLD, "pt")
    cfg = DecoderConfig(**json.loads(f.metadata()["qwen3_like.config"]))
    w = make_weights(cfg, seed=1)
    assert abs(weights_checksum(w) - float(f.metadata()["qwen3_like.weights_checksum"])) < 1e-6 * weights_checksum(w)
    w.update({k[len("qwen3_like."):]: f.get_tensor(k) for k in f.keys() if "_norm.weight" in k})
    return cfg, w, *(torch.stack([f.get_tensor(f"qwen3_like.{n}.{i}") for i in range(4)]) for n in ("generated", "logits"))


def build(cfg, w, wdtype="bf16", kv="auto", qk_norm=1, artifacts=None):
    import vllm_neuron_amd._native as N
    from tests.test_model_gpu import native_model
    orig = N.NativeModel
    N.NativeModel = lambda **kw: orig(qk_norm=qk_norm, kv_cache_dtype=N.MI_KV[kv], **kw)   # native_model() builds the rest
    try:
        return native_model(cfg, w, wdtype, artifacts=artifacts)
    finally:
        N.NativeModel = orig


def run(model, cfg, gen):
    # 4 context encodings (one a prefix-cache hit) over scattered blocks, then 11 teacher-forced steps at B = 4 from a hipGraph
    from tests.test_model_gpu import BS, MAXLEN, MB, NB
    prompts = make_prompts(cfg.vocab_size, 0)
    perm = (torch.randperm(NB - 1, generator=torch.Generator().manual_seed(11)) + 1).tolist()
    blocks = [perm[i * MB:(i + 1) * MB] for i in range(4)]
    blocks[3][0:2] = blocks[1][0:2]
    out = [model.forward(**prefill_inputs(p, blocks[i], BS, MAXLEN, 64 if i == 3 else 0)).clone() for i, p in enumerate(prompts)]
    for s in range(1, gen.shape[1]):
        out.append(model.forward(**decode_inputs(gen[:, s - 1].tolist(), [len(p) + s - 1 for p in prompts], blocks, BS, MAXLEN)).clone())
    return torch.cat([torch.cat(out[:4])[:, None], torch.stack(out[4:], 1)], 1)            # [request, step, V]


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype,kv", [("bf16", "auto"), ("f8e4m3", "auto"), ("bf16", "fp8")])
def test_qwen3_matches_hf_golden(wdtype, kv, tmp_path):
    """Ids equal the golden's wherever its top-2 gap > 0.15; with FP8 KV (unit scales) up to the first step whose gap is
    <= 0.3, the rule of tests/test_kv_fp8_gpu.py; bf16 weights and KV: |logits - HF fp32| <= 0.12."""
    cfg, w, gen, gold = golden()
    model = build(cfg, w, wdtype, kv)
    got = run(model, cfg, gen)
    worst = (got - gold).abs().max().item()
    print(f"{wdtype} weights, {kv} KV: max |device - HF fp32| = {worst:.4f}")
    gap = -gold.topk(2).values.diff(dim=-1)[..., 0]
    need = (gap > 0.3).cumprod(1).bool() if kv == "fp8" else gap > 0.15
    assert (got.argmax(-1) == gen)[need].all(), ((got.argmax(-1) != gen) & need).nonzero().tolist()
    if (wdtype, kv) != ("bf16", "auto"):
        return model.close()
    assert worst <= 0.12, worst
    model.save_artifacts(str(tmp_path))            # the gains are part of the images, qk_norm of their identity
    model.close()
    again = build(cfg, w, artifacts=str(tmp_path))
    assert torch.equal(run(again, cfg, gen), got)
    again.close()
    with pytest.raises(ValueError, match="another model"):
        build(cfg, w, qk_norm=0, artifacts=str(tmp_path))


def test_qwen3_is_accepted_and_configured():
    from vllm_neuron_amd.worker.mi355x_model_loader import _check_architecture, _decoder_geometry
    _check_architecture("Qwen3ForCausalLM")
    geo = _decoder_geometry(SimpleNamespace(model_type="qwen3", num_hidden_layers=2, hidden_size=256, num_attention_heads=4,
                                            num_key_value_heads=2, head_dim=128, intermediate_size=512, vocab_size=512,
                                            rms_norm_eps=1e-6, rope_theta=1e6, attention_bias=False))
    assert (geo["qk_norm"], geo["qkv_bias"], geo["head_dim"]) == (1, 0, 128)
