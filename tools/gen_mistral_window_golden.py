#!/usr/bin/env python3
"""Generate tests/golden/hf_mistral_window_golden.safetensors (dev tool; needs ``transformers`` with Mistral, CPU only).

The sliding-window counterpart of tools/gen_qwen3_golden.py: HF ``MistralForCausalLM`` in fp32 with eager attention,
``sliding_window`` = W and NO KV cache (a full forward over the whole sequence per step) on the seeded synthetic weights of
``oracle.synth.make_weights``.  W is below 64 and no multiple of 16, so the window's lower edge crosses block and tile
borders at odd places.  Four seeded prompts: one shorter than W, one between W and W + 64, two longer than W + 64;
prompts 1 and 3 share their first 70 tokens (a prefix-cache hit of two 32-token blocks).  Recorded per prompt: the prompt,
the 12 greedy ids and the fp32 next-token logits of every step; in the metadata: the geometry ("config", JSON), W and the
checksum of the weights.  The tool asserts that the same model without a window gives other logits on the long prompts:
the fixture cannot be matched by a kernel that ignores the window.

    python tools/gen_mistral_window_golden.py
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
from oracle.synth import make_weights, weights_checksum  # noqa: E402

NAME, NEW_TOKENS, WINDOW = "mistral_like", 12, 24
MISTRAL_LIKE = dict(num_layers=2, hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=64, intermediate_size=512,
                    vocab_size=512, rms_norm_eps=1e-5, rope_theta=10000.0)
LENGTHS = (10, 85, 150, 200)      # stays inside W while it generates; W .. W + 64; > W + 64 twice


def make_prompts(vocab_size: int, seed: int = 3) -> list[list[int]]:
    g = torch.Generator().manual_seed(seed)
    ids = lambda n: torch.randint(0, vocab_size, (n,), generator=g).tolist()  # noqa: E731
    shared = ids(70)
    return [ids(LENGTHS[0]), shared + ids(LENGTHS[1] - 70), ids(LENGTHS[2]), shared + ids(LENGTHS[3] - 70)]


@torch.no_grad()
def main(out_path: str) -> None:
    import transformers
    from transformers import MistralConfig, MistralForCausalLM
    z = MISTRAL_LIKE
    cfg = DecoderConfig(**z)
    w = make_weights(cfg, seed=1)

    def hf_model(window):
        hf_cfg = MistralConfig(vocab_size=z["vocab_size"], hidden_size=z["hidden_size"], intermediate_size=z["intermediate_size"],
                               num_hidden_layers=z["num_layers"], num_attention_heads=z["num_heads"],
                               num_key_value_heads=z["num_kv_heads"], head_dim=z["head_dim"], max_position_embeddings=4096,
                               rms_norm_eps=z["rms_norm_eps"], rope_theta=z["rope_theta"], tie_word_embeddings=False,
                               sliding_window=window, attn_implementation="eager")
        model = MistralForCausalLM(hf_cfg)
        missing, unexpected = model.load_state_dict(w, strict=False)
        assert not unexpected, unexpected
        assert all("rotary" in m or "inv_freq" in m for m in missing), missing
        return model.eval().to(torch.float32)

    model, full = hf_model(WINDOW), hf_model(None)
    tensors = {}
    for i, prompt in enumerate(make_prompts(cfg.vocab_size)):
        seq, step_logits, moved = list(prompt), [], 0.0
        for _ in range(NEW_TOKENS):
            lg = model(torch.tensor([seq]), use_cache=False).logits[0, -1].to(torch.float32)
            moved = max(moved, float((lg - full(torch.tensor([seq]), use_cache=False).logits[0, -1]).abs().max()))
            step_logits.append(lg)
            seq.append(int(lg.argmax()))
        # a prompt inside the window must not see it, one beyond it must -- by far more than the test's 0.12 bar
        assert (moved == 0.0) if len(seq) <= WINDOW else (moved > 1.0), (i, len(prompt), moved)
        tensors[f"{NAME}.prompt.{i}"] = torch.tensor(prompt, dtype=torch.int64)
        tensors[f"{NAME}.generated.{i}"] = torch.tensor(seq[len(prompt):], dtype=torch.int64)
        tensors[f"{NAME}.logits.{i}"] = torch.stack(step_logits)
        top2 = torch.stack(step_logits).topk(2, dim=-1).values
        print(f"{NAME} prompt {i} (len {len(prompt)}): gen {seq[len(prompt):]}  min top1-top2 gap "
              f"{float((top2[:, 0] - top2[:, 1]).min()):.4f}  max |windowed - full| {moved:.3f}")
    meta = {f"{NAME}.config": json.dumps(z), f"{NAME}.sliding_window": str(WINDOW),
            f"{NAME}.weights_checksum": repr(weights_checksum(w)),
            "transformers_version": transformers.__version__, "torch_version": torch.__version__}
    save_file(tensors, out_path, metadata=meta)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(os.path.join(ROOT, "tests", "golden", "hf_mistral_window_golden.safetensors"))
