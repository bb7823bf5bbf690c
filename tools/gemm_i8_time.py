"""Dev tool: what the INT8 x INT8 context-encoding GEMM buys on INT8 weights, timed with HIP events.

    python tools/gemm_i8_time.py [--reps 20] [--markdown]

Per projection shape of Llama-3.1-8B and Qwen2.5-7B at 256 / 512 / 1024 / 2048 rows:
  w8     mi_op_qlinear on INT8 weights, force_path 0: the weight-only GEMM (bf16 MFMA after decode8) as served today
  a8i    mi_op_qlinear_a8_i8: per-token int8 quantization + gemm_a8i_kernel (v_mfma_i32_16x16x64_i8)
  a8f    mi_op_qlinear_a8 on FP8 weights of the same shape: per-token e4m3 quantization + the MX-scaled MFMA GEMM
The two activation-quantizing entry points allocate their image, quantize, launch, synchronize and free inside the call;
mi_op_qlinear only launches.  a8i against a8f is therefore like for like (same host work around the GEMM), a8i against w8
charges the entry point's allocation and synchronization to a8i: the small shapes understate the kernel."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vllm_neuron_amd import _native as lib

SHAPES = [("llama-3.1-8b qkv", 6144, 4096), ("llama-3.1-8b o", 4096, 4096), ("llama-3.1-8b gate+up", 28672, 4096),
          ("llama-3.1-8b down", 4096, 14336), ("qwen2.5-7b qkv", 4608, 3584), ("qwen2.5-7b o", 3584, 3584),
          ("qwen2.5-7b gate+up", 37888, 3584), ("qwen2.5-7b down", 3584, 18944)]
ROWS = [256, 512, 1024, 2048]


def timed(launch, reps):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without one"
    L = lib.load_library()
    sep = " | " if args.markdown else "  "
    head = ["shape", "N", "K", "rows", "w8 us", "a8i us", "a8f us", "w8 / a8i", "a8f / a8i", "a8i Top/s"]
    print(("| " if args.markdown else "") + sep.join(head) + (" |" if args.markdown else ""))
    if args.markdown:
        print("|" + "---|" * len(head))
    for name, N, K in SHAPES:
        wi = torch.randint(-127, 128, (N * K,), dtype=torch.int8, device="cuda")      # codes; the tile order does not matter to a timing
        wf = torch.randint(0, 0x70, (N * K,), dtype=torch.uint8, device="cuda")       # e4m3 codes, no NaN
        scale = torch.full((N,), 1e-3, dtype=torch.float32, device="cuda")
        for M in ROWS:
            x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            y = torch.empty(M, N, dtype=torch.float32, device="cuda")
            w8 = timed(lambda: lib.check(L.mi_op_qlinear(x.data_ptr(), M, wi.data_ptr(), scale.data_ptr(), None, N, K, 2,
                                                         y.data_ptr(), 0, None)), args.reps)
            a8i = timed(lambda: lib.check(L.mi_op_qlinear_a8_i8(x.data_ptr(), M, wi.data_ptr(), scale.data_ptr(), None, N, K, 0,
                                                                y.data_ptr(), None)), args.reps)
            a8f = timed(lambda: lib.check(L.mi_op_qlinear_a8(x.data_ptr(), M, wf.data_ptr(), scale.data_ptr(), None, N, K,
                                                             y.data_ptr(), None)), args.reps)
            row = [name, str(N), str(K), str(M), f"{w8:.1f}", f"{a8i:.1f}", f"{a8f:.1f}", f"{w8 / a8i:.2f}", f"{a8f / a8i:.2f}",
                   f"{2.0 * M * N * K / a8i / 1e6:.0f}"]
            print(("| " if args.markdown else "") + sep.join(row) + (" |" if args.markdown else ""), flush=True)


if __name__ == "__main__":
    main()
