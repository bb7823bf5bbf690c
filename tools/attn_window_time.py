"""Sliding-window attention against the unwindowed kernels on the same pool (dev tool, not a test).

Llama-3.1-8B / Mistral-7B head geometry (nh 32, nkv 8, hd 128, block 32), scattered blocks, window 4096, a bf16 pool and an
FP8 (e4m3) pool holding the same values:
  decode   B 4 x ctx 16384 (the window skips 3/4 of the tiles) and B 32 x ctx 1024 (inside the window: the same tiles)
           plain   mi_op_paged_attn_decode / mi_op_paged_attn_decode_f8
           window  mi_op_paged_attn_decode_sw
  prefill  T 512 at pos0 15872 (a late chunk: a band of ~72 of 256 tiles) and T 2048 at pos0 0 (inside the window: the launcher
           takes the unwindowed kernel)
           plain   mi_op_paged_attn_prefill; FP8: mi_op_kv_dequant_gather of the whole prefix + the same on the staged copy
           window  mi_op_paged_attn_prefill_sw; FP8: the gather of the blocks the band touches + the same on the staged copy
Device events: warm-up, then ROUNDS rounds of ITERS launches per form, the forms alternating; prints the median and the
min / max over the rounds."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vllm_neuron_amd import _native as N

NH, NKV, HD, BS, W = 32, 8, 128, 32, 4096
ROUNDS, ITERS = 9, 20
lib = N.load_library()


def pools(nb, g):
    codes = torch.randn(2, nb, NKV, BS, HD, device="cuda", generator=g).clamp(-448, 448).to(torch.float8_e4m3fn)
    return {"bf16": codes.to(torch.bfloat16), "fp8": codes.view(torch.uint8)}


def report(title, forms):
    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / ITERS      # us per call

    for fn in forms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in forms}
    for _ in range(ROUNDS):
        for name, fn in forms.items():
            t[name].append(timed(fn))
    for name in forms:
        print(f"{title} {name:6s}: median {statistics.median(t[name]):8.2f} us  (min {min(t[name]):.2f}, max {max(t[name]):.2f})",
              flush=True)


def decode(B, ctx):
    MB = (ctx + BS - 1) // BS
    nb = 1 + B * MB
    g = torch.Generator(device="cuda").manual_seed(1)
    pool = pools(nb, g)
    bt = (torch.randperm(nb - 1, device="cuda", generator=g) + 1).int().reshape(B, MB).contiguous()
    cl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    q = torch.randn(B, NH, HD, device="cuda", generator=g).to(torch.bfloat16)
    out = torch.empty(B, NH * HD, dtype=torch.bfloat16, device="cuda")
    scratch = torch.empty(lib.mi_op_attn_scratch_bytes(B, NH, HD), dtype=torch.uint8, device="cuda")
    for kv in ("bf16", "fp8"):
        head = (q.data_ptr(), pool[kv].data_ptr(), nb, BS, bt.data_ptr(), MB, cl.data_ptr(), B, NH, NKV, HD)
        tail = (out.data_ptr(), scratch.data_ptr(), None)
        plain = (lambda: N.check(lib.mi_op_paged_attn_decode_f8(*head, 1.0, 1.0, *tail))) if kv == "fp8" else \
                (lambda: N.check(lib.mi_op_paged_attn_decode(*head, *tail)))
        window = lambda: N.check(lib.mi_op_paged_attn_decode_sw(*head, int(kv == "fp8"), 1.0, 1.0, W, *tail))  # noqa: E731
        report(f"decode  B {B:2d} ctx {ctx:5d} W {W} {kv:4s}", {"plain": plain, "window": window})


def prefill(T, pos0):
    kv_len = pos0 + T
    MB = (kv_len + BS - 1) // BS
    nb = 1 + MB
    g = torch.Generator(device="cuda").manual_seed(1)
    pool = pools(nb, g)
    bt = (torch.randperm(nb - 1, device="cuda", generator=g) + 1).int().contiguous()
    q = torch.randn(T, NH, HD, device="cuda", generator=g).to(torch.bfloat16)
    out = torch.empty(T, NH * HD, dtype=torch.bfloat16, device="cuda")
    args = lambda p, nblk, table: (q.data_ptr(), T, pos0, p.data_ptr(), nblk, BS, table.data_ptr(), MB, NH, NKV, HD)  # noqa: E731
    report(f"prefill T {T:4d} pos0 {pos0:5d} W {W} bf16", {
        "plain": lambda: N.check(lib.mi_op_paged_attn_prefill(*args(pool["bf16"], nb, bt), out.data_ptr(), None)),
        "window": lambda: N.check(lib.mi_op_paged_attn_prefill_sw(*args(pool["bf16"], nb, bt), W, out.data_ptr(), None))})
    # FP8: the staged copy.  The windowed form stages the blocks from the first tile of the band on (what a context does);
    # here they land in a pool of their own, so the table is the identity shifted by the first staged block.
    blk0 = (max(pos0 - W + 1, 0) // 64 * 64) // BS if kv_len > W else 0
    staged = torch.empty(2, MB, NKV, BS, HD, dtype=torch.bfloat16, device="cuda")
    ident = torch.arange(MB, dtype=torch.int32, device="cuda")
    shifted, tail_bt = (ident - blk0).clamp(min=0).contiguous(), bt[blk0:].contiguous()

    def plain8():
        N.check(lib.mi_op_kv_dequant_gather(pool["fp8"].data_ptr(), nb, BS, bt.data_ptr(), MB, kv_len, NKV, HD, 1.0, 1.0,
                                            staged.data_ptr(), None))
        N.check(lib.mi_op_paged_attn_prefill(*args(staged, MB, ident), out.data_ptr(), None))

    def window8():
        N.check(lib.mi_op_kv_dequant_gather(pool["fp8"].data_ptr(), nb, BS, tail_bt.data_ptr(), MB - blk0, kv_len - blk0 * BS,
                                            NKV, HD, 1.0, 1.0, staged.data_ptr(), None))
        N.check(lib.mi_op_paged_attn_prefill_sw(*args(staged, MB - blk0, shifted), W, out.data_ptr(), None))

    report(f"prefill T {T:4d} pos0 {pos0:5d} W {W} fp8 ", {"plain": plain8, "window": window8})


decode(4, 16384)
decode(32, 1024)
prefill(512, 15872)
prefill(2048, 0)
