#!/usr/bin/env python3
"""Generate tests/golden/hf_qwen3_golden.safetensors (dev tool; needs ``transformers`` with Qwen3, CPU only).

The Qwen3 counterpart of oracle/gen_golden.py: HF ``Qwen3ForCausalLM`` in fp32 with eager attention and NO KV cache
(a full forward over the whole sequence per step) on the seeded synthetic weights of ``oracle.synth.make_weights`` plus
seeded bf16-representable q_norm / k_norm gains, which the decoder zoo has no notion of and which are therefore stored
in the fixture.  Recorded per prompt: the prompt, the 12 greedy ids and the fp32 next-token logits of every step; in the
metadata: the geometry ("config", JSON) and the checksum of the make_weights tensors.

    python tools/gen_qwen3_golden.py
"""

from __future__ import annotations

import json
import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.paged_decoder import DecoderConfig  # noqa: E402
from oracle.synth import make_prompts, make_weights, weights_checksum  # noqa: E402

NAME, NEW_TOKENS = "qwen3_like", 12
# q_dim = 4 * 128 = 512 != hidden_size: head_dim is its own quantity, as in every Qwen3 checkpoint
QWEN3_LIKE = dict(num_layers=2, hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=128, intermediate_size=512,
                  vocab_size=512, rms_norm_eps=1e-6, rope_theta=1000000.0)


def make_gains(cfg: DecoderConfig, seed: int = 2) -> dict:
    g = torch.Generator().manual_seed(seed)
    return {f"model.layers.{l}.self_attn.{n}_norm.weight":
            (1.0 + 0.1 * torch.randn(cfg.head_dim, generator=g)).to(torch.bfloat16).to(torch.float32)
            for l in range(cfg.num_layers) for n in ("q", "k")}


@torch.no_grad()
def main(out_path: str) -> None:
    import transformers
    from transformers import Qwen3Config, Qwen3ForCausalLM
    z = QWEN3_LIKE
    cfg = DecoderConfig(**z)
    hf_cfg = Qwen3Config(vocab_size=z["vocab_size"], hidden_size=z["hidden_size"], intermediate_size=z["intermediate_size"],
                         num_hidden_layers=z["num_layers"], num_attention_heads=z["num_heads"],
                         num_key_value_heads=z["num_kv_heads"], head_dim=z["head_dim"], max_position_embeddings=4096,
                         rms_norm_eps=z["rms_norm_eps"], rope_theta=z["rope_theta"], tie_word_embeddings=False,
                         attention_bias=False, use_sliding_window=False, attn_implementation="eager")
    model = Qwen3ForCausalLM(hf_cfg)
    w, gains = make_weights(cfg, seed=1), make_gains(cfg)
    missing, unexpected = model.load_state_dict({**w, **gains}, strict=False)
    assert not unexpected, unexpected
    assert all("rotary" in m or "inv_freq" in m for m in missing), missing
    model = model.eval().to(torch.float32)
    tensors = {f"{NAME}.{k}": v for k, v in gains.items()}
    for i, prompt in enumerate(make_prompts(cfg.vocab_size, seed=0)):
        seq, step_logits = list(prompt), []
        for _ in range(NEW_TOKENS):
            lg = model(torch.tensor([seq]), use_cache=False).logits[0, -1].to(torch.float32)
            step_logits.append(lg)
            seq.append(int(lg.argmax()))
        tensors[f"{NAME}.prompt.{i}"] = torch.tensor(prompt, dtype=torch.int64)
        tensors[f"{NAME}.generated.{i}"] = torch.tensor(seq[len(prompt):], dtype=torch.int64)
        tensors[f"{NAME}.logits.{i}"] = torch.stack(step_logits)
        top2 = torch.stack(step_logits).topk(2, dim=-1).values
        print(f"{NAME} prompt {i} (len {len(prompt)}): gen {seq[len(prompt):]}  "
              f"min top1-top2 gap {float((top2[:, 0] - top2[:, 1]).min()):.4f}")
    meta = {f"{NAME}.config": json.dumps(z), f"{NAME}.weights_checksum": repr(weights_checksum(w)),
            "transformers_version": transformers.__version__, "torch_version": torch.__version__}
    save_file(tensors, out_path, metadata=meta)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(os.path.join(ROOT, "tests", "golden", "hf_qwen3_golden.safetensors"))
