"""Mistral (sliding-window attention) end to end against the committed HF-transformers golden
(tools/gen_mistral_window_golden.py: window 24, prompts of 10 / 85 / 150 / 200 tokens, 12 greedy steps)."""

import json
import os
from types import SimpleNamespace
from unittest import mock

import pytest
import torch
from safetensors import safe_open

from oracle.paged_decoder import DecoderConfig
from oracle.synth import make_weights, weights_checksum
from tests.helpers import decode_inputs, prefill_inputs

GOLD = os.path.join(os.path.dirname(__file__), "golden", "hf_mistral_window_golden.safetensors")


def golden():   # -> (config, weights, window, prompts [4], greedy ids [4, 12], fp32 logits [4, 12, V])
    f, n = safe_open(GOLD, "pt"), "mistral_like"
    cfg = DecoderConfig(**json.loads(f.metadata()[f"{n}.config"]))
    w = make_weights(cfg, seed=1)
    assert abs(weights_checksum(w) - float(f.metadata()[f"{n}.weights_checksum"])) < 1e-6 * weights_checksum(w)
    gen, gold = (torch.stack([f.get_tensor(f"{n}.{what}.{i}") for i in range(4)]) for what in ("generated", "logits"))
    return cfg, w, int(f.metadata()[f"{n}.sliding_window"]), [f.get_tensor(f"{n}.prompt.{i}").tolist() for i in range(4)], gen, gold


def windowed(builder, window, kv="auto"):   # builder() with sliding_window / kv_cache_dtype added to the NativeModel it constructs
    import vllm_neuron_amd._native as N
    orig = N.NativeModel
    with mock.patch.object(N, "NativeModel", lambda **kw: orig(sliding_window=window, kv_cache_dtype=N.MI_KV[kv], **kw)):
        return builder()


def run(model, prompts, gen):
    # 4 context encodings (one a prefix-cache hit) over scattered blocks, then 11 teacher-forced steps at B = 4 from a hipGraph
    from tests.test_model_gpu import BS, MAXLEN, MB, NB
    perm = (torch.randperm(NB - 1, generator=torch.Generator().manual_seed(11)) + 1).tolist()
    blocks = [perm[i * MB:(i + 1) * MB] for i in range(4)]
    blocks[3][0:2] = blocks[1][0:2]
    out = [model.forward(**prefill_inputs(p, blocks[i], BS, MAXLEN, 64 if i == 3 else 0)).clone() for i, p in enumerate(prompts)]
    for s in range(1, gen.shape[1]):
        out.append(model.forward(**decode_inputs(gen[:, s - 1].tolist(), [len(p) + s - 1 for p in prompts], blocks, BS, MAXLEN)).clone())
    model.close()
    return torch.cat([torch.cat(out[:4])[:, None], torch.stack(out[4:], 1)], 1)            # [request, step, V]


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype,kv", [("bf16", "auto"), ("f8e4m3", "auto"), ("bf16", "fp8")])
def test_mistral_window_matches_hf_golden(wdtype, kv):
    """The rules of tests/test_qwen3_gpu.py (gap > 0.15; FP8 KV: up to the first gap <= 0.3; bf16: |logits - HF fp32| <= 0.12,
    DESIGN 2), a bar the same weights without the window miss on every prompt longer than it."""
    from tests.test_model_gpu import native_model
    cfg, w, W, prompts, gen, gold = golden()
    got = run(windowed(lambda: native_model(cfg, w, wdtype), W, kv), prompts, gen)
    worst = (got - gold).abs().amax((1, 2))
    gap = -gold.topk(2).values.diff(dim=-1)[..., 0]
    need = (gap > 0.3).cumprod(1).bool() if kv == "fp8" else gap > 0.15
    assert (got.argmax(-1) == gen)[need].all(), ((got.argmax(-1) != gen) & need).nonzero().tolist()
    if (wdtype, kv) == ("bf16", "auto"):
        assert worst.max() <= 0.12, worst.tolist()
        miss = (run(windowed(lambda: native_model(cfg, w), 0), prompts, gen) - gold).abs().amax((1, 2))
        assert miss[0] <= 0.12 and (miss[1:] > 0.12).all(), miss.tolist()


@pytest.mark.gpu
def test_mistral_window_fused_speculation():
    """Windowed target + copied windowed draft, k = 4 (R > 1: one lower edge per MFMA column).  Generation runs free, so a
    request is held to the golden's ids up to the first step whose top-2 gap is <= 0.15: behind a near-tie the texts may part."""
    from oracle.spec_decode import remask
    from tests.test_spec_decode_gpu import BS, MAXLEN, MB, NSEQ, K, _Catchup, _model
    cfg, w, W, prompts, gen, gold = golden()
    target, draft = windowed(lambda: _model(cfg, w, NSEQ * K), W), windowed(lambda: _model(cfg, w, 2 * NSEQ), W)
    blocks = [[1 + i * MB + j for j in range(MB)] for i in range(NSEQ)]
    got = []
    for inp in (prefill_inputs(p, blocks[i], BS, MAXLEN, 0) for i, p in enumerate(prompts)):
        got.append([int(target.forward(**inp).argmax(dim=1)[0])])
        draft.forward(**inp)
    bt, cu, n_new = torch.tensor(blocks, dtype=torch.long), _Catchup(NSEQ), gen.shape[1]
    while min(len(g) for g in got) < n_new:
        last = torch.tensor([g[-1] for g in got])
        pos = torch.tensor([len(p) + len(g) - 1 for p, g in zip(prompts, got)])
        acc, nxt = target.forward_spec(draft, last, pos, bt, K, catchup_ids=cu.ids(pos))
        cu.record(pos, acc, nxt, K)
        for i, row in enumerate(remask(acc, nxt, pos)):
            got[i].extend(int(t) for t in row if t != -1)
    draft.close()
    target.close()
    need = (-gold.topk(2).values.diff(dim=-1)[..., 0] > 0.15).cumprod(1).bool()
    ids = torch.tensor([g[:n_new] for g in got])
    assert need[1:].sum() > 0 and (ids == gen)[need].all(), ((ids != gen) & need).nonzero().tolist()


def test_loader_reads_the_window_of_mistral_only():
    from vllm_neuron_amd.worker.mi355x_model_loader import _decoder_geometry
    base = dict(num_hidden_layers=2, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
                vocab_size=512, rms_norm_eps=1e-5, rope_theta=1e4)
    geo = lambda **kw: _decoder_geometry(SimpleNamespace(**base, **kw))["sliding_window"]  # noqa: E731
    assert geo(model_type="mistral", sliding_window=4096) == 4096 and geo(model_type="llama") == 0
    assert geo(model_type="qwen2", use_sliding_window=True, sliding_window=4096, max_window_layers=1) == 0
