"""The Qwen3 per-head QK-norm kernel, timed (dev tool, not a test).

(a) mi_op_qk_norm_rope_kv alone at nh 32 / nkv 8 / hd 128 for T in {4, 32, 2048}, bf16 and FP8 pool: device events,
    warm-up, ROUNDS rounds of ITERS launches per form, the two forms alternating; median, min / max, bytes moved.
(b) the token-generation step at Qwen3-8B geometry (36 layers, H 4096, I 12288, vocab 151936, FP8 weights, synthetic),
    B 4 at context 1024, qk_norm 1 against 0 on the same build: graph replays (mi_replay_decode), alternating rounds.
    The difference is the price of the extra launch (and of the fp32 round trip of q|k|v) per layer."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tests.helpers import decode_inputs
from vllm_neuron_amd import _native as N

NH, NKV, HD, BS, NB = 32, 8, 128, 32, 129
ROUNDS, ITERS = 9, 50
lib = N.load_library()


def stats(v):
    return f"median {statistics.median(v):8.3f}  (min {min(v):.3f}, max {max(v):.3f})"


def kernel_case(T):
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv = torch.randn(T, (NH + 2 * NKV) * HD, device="cuda", generator=g)
    gq, gk = torch.ones(HD, device="cuda"), torch.ones(HD, device="cuda")
    pos = torch.randint(0, 4096, (T,), device="cuda", generator=g, dtype=torch.int32)
    slots = (torch.randperm((NB - 1) * BS, device="cuda", generator=g)[:T] + BS).int()
    cos, sin = torch.rand(4096, HD // 2, device="cuda"), torch.rand(4096, HD // 2, device="cuda")
    q = torch.empty(T, NH * HD, dtype=torch.bfloat16, device="cuda")
    pools = {0: torch.zeros(2, NB, NKV, BS, HD, dtype=torch.bfloat16, device="cuda"),
             1: torch.zeros(2, NB, NKV, BS, HD, dtype=torch.uint8, device="cuda")}

    def timed(kv):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            N.check(lib.mi_op_qk_norm_rope_kv(qkv.data_ptr(), gq.data_ptr(), gk.data_ptr(), pos.data_ptr(), slots.data_ptr(), T,
                                              NH, NKV, HD, 1e-6, cos.data_ptr(), sin.data_ptr(), q.data_ptr(),
                                              pools[kv].data_ptr(), NB, BS, kv, 1.0, 1.0, None))
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / ITERS
    for kv in (0, 1, 0, 1):
        timed(kv)
    t = {0: [], 1: []}
    for _ in range(ROUNDS):
        for kv in (0, 1):
            t[kv].append(timed(kv))
    for kv, name in ((0, "bf16"), (1, "fp8")):
        kb = T * ((NH + 2 * NKV) * HD * 4 + NH * HD * 2 + 2 * NKV * HD * (1 if kv else 2) + HD * 4) / 1e3   # fp32 q|k|v in, q + K + V out, one cos / sin row
        print(f"kernel T {T:5d} {name:5s} pool: {stats(t[kv])} us   {kb:9.1f} KB moved", flush=True)


def step_case():
    geo = dict(num_layers=36, hidden_size=4096, num_heads=NH, num_kv_heads=NKV, head_dim=HD, intermediate_size=12288,
               vocab_size=151936, rms_norm_eps=1e-6, rope_theta=1e6, rope_factor=1.0, rope_low_freq_factor=1.0,
               rope_high_freq_factor=4.0)
    B, ctx, maxlen = 4, 1024, 2048
    mb = maxlen // BS
    blocks = [[1 + b * mb + j for j in range(mb)] for b in range(B)]
    models = {}
    for qn in (0, 1):
        m = N.NativeModel(num_blocks=1 + B * mb, block_size=BS, max_num_seqs=B, max_model_len=maxlen, weight_dtype=N.MI_W["fp8"],
                          quant_type=N.MI_Q["per_channel_symmetric"], quantize_lm_head=1, tp_degree=1, tp_rank=0, device_id=0,
                          use_graphs=1, qk_norm=qn, **geo)
        m.init_synthetic_weights(1, 0.02)
        m.finalize()
        for _ in range(2):   # the second call replays the captured graph
            m.forward(**decode_inputs([1] * B, [ctx - 1] * B, blocks, BS, maxlen))
        m.replay_decode(20)
        models[qn] = m
    t = {0: [], 1: []}
    for _ in range(ROUNDS):
        for qn in (0, 1):
            t[qn].append(models[qn].replay_decode(ITERS) / ITERS)
    for qn in (0, 1):
        print(f"decode step B {B} ctx {ctx} qk_norm {qn}: {stats(t[qn])} ms", flush=True)
    d = (statistics.median(t[1]) - statistics.median(t[0])) * 1e3
    print(f"qk_norm 1 - 0: {d:.1f} us per step = {d / geo['num_layers']:.2f} us per layer", flush=True)


for T in (4, 32, 2048):
    kernel_case(T)
step_case()
