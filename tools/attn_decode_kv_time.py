"""Decode attention over a bf16 pool against an FP8 (e4m3) pool (dev tool, not a test).

Times mi_op_paged_attn_decode and mi_op_paged_attn_decode_f8 at the Llama-3.1-8B head geometry
(nh 32, nkv 8, hd 128, block 32) with device events: warm-up, then ROUNDS rounds of ITERS launches
per kernel, the two kernels alternating; prints the median and the min / max over the rounds, the
bytes of K/V each form reads, and the largest difference between the two outputs (same values in
both pools: codes dequantised with unit scales)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vllm_neuron_amd import _native as N

NH, NKV, HD, BS = 32, 8, 128, 32
ROUNDS, ITERS = 9, 50
lib = N.load_library()


def case(B, ctx):
    MB = ctx // BS
    nb = 1 + B * MB
    g = torch.Generator(device="cuda").manual_seed(1)
    codes = torch.randn(2, nb, NKV, BS, HD, device="cuda", generator=g).clamp(-448, 448).to(torch.float8_e4m3fn)
    pool8, pool16 = codes.view(torch.uint8), codes.to(torch.bfloat16)        # the same values in both pools
    bt = (torch.randperm(nb - 1, device="cuda", generator=g) + 1).int().reshape(B, MB).contiguous()
    cl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    q = torch.randn(B, NH, HD, device="cuda", generator=g).to(torch.bfloat16)
    scratch = torch.empty(lib.mi_op_attn_scratch_bytes(B, NH, HD), dtype=torch.uint8, device="cuda")
    o16, o8 = (torch.empty(B, NH * HD, dtype=torch.bfloat16, device="cuda") for _ in range(2))

    def bf16():
        N.check(lib.mi_op_paged_attn_decode(q.data_ptr(), pool16.data_ptr(), nb, BS, bt.data_ptr(), MB, cl.data_ptr(), B, NH,
                                            NKV, HD, o16.data_ptr(), scratch.data_ptr(), None))

    def fp8():
        N.check(lib.mi_op_paged_attn_decode_f8(q.data_ptr(), pool8.data_ptr(), nb, BS, bt.data_ptr(), MB, cl.data_ptr(), B, NH,
                                               NKV, HD, 1.0, 1.0, o8.data_ptr(), scratch.data_ptr(), None))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / ITERS      # us per launch (split + combine where the grid is short)

    for fn in (bf16, fp8):
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    t = {"bf16": [], "fp8": []}
    for _ in range(ROUNDS):
        t["bf16"].append(timed(bf16))
        t["fp8"].append(timed(fp8))
    diff = (o16.float() - o8.float()).abs().max().item()
    for name, width in (("bf16", 2), ("fp8", 1)):
        mb = 2 * B * ctx * NKV * HD * width / 1e6
        med = statistics.median(t[name])
        print(f"B {B:3d} ctx {ctx:6d} {name:5s}: median {med:8.2f} us  (min {min(t[name]):.2f}, max {max(t[name]):.2f})  "
              f"K/V {mb:8.1f} MB -> {mb / med * 1e3:7.0f} GB/s", flush=True)
    print(f"B {B:3d} ctx {ctx:6d} max |bf16 - fp8| = {diff:.4f}", flush=True)


for B, ctx in ((4, 1024), (32, 1024), (4, 16384)):
    case(B, ctx)
