"""Context-encoding attention over a bf16 pool against an FP8 (e4m3) pool, staged and native (dev tool, not a test).

Three forms at the Llama-3.1-8B head geometry (nh 32, nkv 8, hd 128, block 32), scattered blocks, the same values
in both pools (codes dequantised with unit scales):
  bf16    mi_op_paged_attn_prefill on the bf16 pool
  staged  mi_op_kv_dequant_gather of the whole prefix + mi_op_paged_attn_prefill on the staged copy (identity table)
  native  mi_op_paged_attn_prefill_f8 on the byte pool
Device events: warm-up, then ROUNDS rounds of ITERS launches per form, the forms alternating; prints the median and
the min / max over the rounds and the largest difference of each FP8 form's output from the bf16 form's."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vllm_neuron_amd import _native as N

NH, NKV, HD, BS = 32, 8, 128, 32
ROUNDS, ITERS = 9, 20
lib = N.load_library()


def case(T, pos0):
    kv_len = pos0 + T
    MB = (kv_len + BS - 1) // BS
    nb = 1 + MB
    g = torch.Generator(device="cuda").manual_seed(1)
    codes = torch.randn(2, nb, NKV, BS, HD, device="cuda", generator=g).clamp(-448, 448).to(torch.float8_e4m3fn)
    pool8, pool16 = codes.view(torch.uint8), codes.to(torch.bfloat16)        # the same values in both pools
    bt = (torch.randperm(nb - 1, device="cuda", generator=g) + 1).int().contiguous()
    ident = torch.arange(MB, dtype=torch.int32, device="cuda")
    staged = torch.empty(2, MB, NKV, BS, HD, dtype=torch.bfloat16, device="cuda")
    q = torch.randn(T, NH, HD, device="cuda", generator=g).to(torch.bfloat16)
    out = {name: torch.empty(T, NH * HD, dtype=torch.bfloat16, device="cuda") for name in ("bf16", "staged", "native")}

    def bf16():
        N.check(lib.mi_op_paged_attn_prefill(q.data_ptr(), T, pos0, pool16.data_ptr(), nb, BS, bt.data_ptr(), MB, NH, NKV, HD,
                                             out["bf16"].data_ptr(), None))

    def staged_form():
        N.check(lib.mi_op_kv_dequant_gather(pool8.data_ptr(), nb, BS, bt.data_ptr(), MB, kv_len, NKV, HD, 1.0, 1.0,
                                            staged.data_ptr(), None))
        N.check(lib.mi_op_paged_attn_prefill(q.data_ptr(), T, pos0, staged.data_ptr(), MB, BS, ident.data_ptr(), MB, NH, NKV,
                                             HD, out["staged"].data_ptr(), None))

    def native():
        N.check(lib.mi_op_paged_attn_prefill_f8(q.data_ptr(), T, pos0, pool8.data_ptr(), nb, BS, bt.data_ptr(), MB, NH, NKV,
                                                HD, 1.0, 1.0, out["native"].data_ptr(), None))

    forms = {"bf16": bf16, "staged": staged_form, "native": native}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / ITERS      # us per call (gather + attention for the staged form)

    for fn in forms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in forms}
    for _ in range(ROUNDS):
        for name, fn in forms.items():
            t[name].append(timed(fn))
    for name in forms:
        med = statistics.median(t[name])
        diff = (out[name].float() - out["bf16"].float()).abs().max().item()
        print(f"T {T:5d} pos0 {pos0:6d} {name:6s}: median {med:8.2f} us  (min {min(t[name]):.2f}, max {max(t[name]):.2f})  "
              f"max |out - bf16 form| = {diff:.4f}", flush=True)


for T, pos0 in ((2048, 0), (512, 15872), (256, 0)):
    case(T, pos0)
