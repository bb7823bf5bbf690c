"""Dev tool: what MXFP4 weights buy against FP8 weights, timed with HIP events.

    python tools/gemv_w4_time.py [--reps 200] [--steps 100] [--markdown] [--no-model]

Per projection shape of Llama-3.1-8B at 4 / 16 / 32 rows (token generation: gemv_w4_kernel against the FP8 GEMV kernels)
and 512 rows (context encoding: gemm_w4_kernel against the FP8 weight-only GEMM), mi_op_qlinear with force_path 0 on both.
The weight image of one call is 17 / 32 of the FP8 image (N K / 2 codes + N K / 32 scales against N K): `ratio` is
fp8 us / mxfp4 us, 1.88 if the stream were all there is.  GB/s is the MXFP4 image over the MXFP4 time.
Then mi_replay_decode (the captured token-generation step, 4 rows) of a synthetic-weight Llama-3.1-8B context per dtype.
Every shape is warmed up before its timed window; the two dtypes of a shape are timed back to back."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vllm_neuron_amd import _native as lib

SHAPES = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate+up", 28672, 4096), ("down", 4096, 14336), ("lm_head", 128256, 4096)]
ROWS = [4, 16, 32, 512]
LLAMA_8B = dict(num_layers=32, hidden_size=4096, num_heads=32, num_kv_heads=8, head_dim=128, intermediate_size=14336,
                vocab_size=128256, rms_norm_eps=1e-5, rope_theta=500000.0, rope_type=0, rope_factor=1.0, rope_low_freq_factor=1.0,
                rope_high_freq_factor=4.0, rope_original_max_position=0, qkv_bias=0, tie_word_embeddings=0)


def image_bytes(N, K, wd):
    return N * K // 2 + N * ((K + 511) // 512) * 16 if wd == 3 else N * K


def timed(launch, reps):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def decode_step_ms(wd, steps):
    m = lib.NativeModel(num_blocks=65, block_size=32, max_num_seqs=4, max_model_len=512, weight_dtype=wd, quant_type=1,
                        quantize_lm_head=1, tp_degree=1, tp_rank=0, device_id=0, use_graphs=1, **LLAMA_8B)
    try:
        m.init_synthetic_weights(seed=1, std=0.02)
        m.finalize()
        B, mb = 4, 16
        ids = torch.randint(0, 1000, (B, 1), dtype=torch.long)
        pos = torch.full((B, 1), 100, dtype=torch.long)
        bt = torch.arange(1, 1 + B * mb, dtype=torch.long).reshape(B, mb)
        slots = (bt[:, 3] * 32 + 4).reshape(B, 1)
        for _ in range(3):     # captures the step
            m.forward(input_ids=ids, position_ids=pos, seq_ids=torch.arange(B), block_table=bt, slot_mapping=slots,
                      full_context_lens=pos + 1, computed_context_lens=pos)
        m.replay_decode(10)
        return m.replay_decode(steps) / steps, m.kv_stats()["weight_bytes"]
    finally:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--no-model", action="store_true", help="skip the two 8B contexts")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without one"
    L = lib.load_library()
    sep = " | " if args.markdown else "  "
    head = ["shape", "N", "K", "rows", "fp8 us", "mxfp4 us", "ratio", "mxfp4 GB/s"]
    print(("| " if args.markdown else "") + sep.join(head) + (" |" if args.markdown else ""))
    if args.markdown:
        print("|" + "---|" * len(head))
    for name, N, K in SHAPES:
        # random codes; every byte pattern is a finite value in both formats below (e4m3 codes < 0x70, e8m0 scale bytes near 2^0)
        w8 = torch.randint(0, 0x70, (N * K,), dtype=torch.uint8, device="cuda")
        w4 = torch.randint(0, 256, (image_bytes(N, K, 3),), dtype=torch.uint8, device="cuda")
        w4[N * K // 2:] = torch.randint(120, 128, (w4.numel() - N * K // 2,), dtype=torch.uint8, device="cuda")
        scale = torch.full((N,), 1e-3, dtype=torch.float32, device="cuda")
        for M in ROWS:
            x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            y = torch.empty(M, N, dtype=torch.float32, device="cuda")
            reps = args.reps if M <= 32 else max(args.reps // 10, 5)
            t8 = timed(lambda: lib.check(L.mi_op_qlinear(x.data_ptr(), M, w8.data_ptr(), scale.data_ptr(), None, N, K, 1,
                                                         y.data_ptr(), 0, None)), reps)
            t4 = timed(lambda: lib.check(L.mi_op_qlinear(x.data_ptr(), M, w4.data_ptr(), scale.data_ptr(), None, N, K, 3,
                                                         y.data_ptr(), 0, None)), reps)
            row = [name, str(N), str(K), str(M), f"{t8:.1f}", f"{t4:.1f}", f"{t8 / t4:.2f}", f"{image_bytes(N, K, 3) / t4 / 1e3:.0f}"]
            print(("| " if args.markdown else "") + sep.join(row) + (" |" if args.markdown else ""), flush=True)
    if not args.no_model:
        for name, wd in (("f8e4m3", 1), ("mxfp4", 3)):
            ms, wb = decode_step_ms(wd, args.steps)
            print(f"llama-3.1-8b synthetic, 4 rows, {name}: {ms:.3f} ms per replayed decode step, weight_bytes {wb / 2**30:.2f} GiB", flush=True)


if __name__ == "__main__":
    main()
