"""Dev tool: what FP8 activations buy on MXFP4 weights in context encoding.

    python tools/gemm_w4a8_time.py [--reps 20] [--windows 3] [--markdown]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gemm_w4a8_time.py --reps 20 --windows 1
    python tools/gemm_w4a8_time.py --from-trace DIR/.../*_kernel_trace.csv [--markdown]

Per projection shape of Llama-3.1-8B at 256 / 512 / 1024 / 2048 rows, mi_op_qlinear on one MXFP4 image:
  w4     force_path 2: gemm_w4_kernel, every code decoded to bf16 (v_cvt_scalef32_pk_bf16_fp4), bf16 MFMA
  a8w4   force_path 8: per-token e4m3 quantization + gemm_a8w4_kernel (codes and scale words as stored into the MX-scaled MFMA)
The first form times calls with HIP events, the two paths alternating window by window (median and spread over the windows).
force_path 8 allocates its image, quantizes, launches, synchronizes and frees inside the call while force_path 2 only
launches, so the call times charge the entry point's host work to a8w4.  The kernel times come from the second form: a
kernel trace of this very program (in a run of its own: tracing slows the host), read back by the third, which sums the
device time of each call's kernels (w4: GEMM + K-split sum; a8w4: row quantizer + GEMM + K-split sum) after the warm-up."""
import argparse
import csv
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate+up", 28672, 4096), ("down", 4096, 14336)]
ROWS = [256, 512, 1024, 2048]
WARM = 3


def table(rows, head, markdown):
    sep = " | " if markdown else "  "
    edge = ("| ", " |") if markdown else ("", "")
    print(edge[0] + sep.join(head) + edge[1])
    if markdown:
        print("|" + "---|" * len(head))
    for r in rows:
        print(edge[0] + sep.join(r) + edge[1], flush=True)


def from_trace(path, reps, markdown):
    """Dispatches in time order; a call is the kernels up to and including its GEMM's K-split sum (if any)."""
    with open(path, newline="") as f:
        recs = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)))
    seg, cur = [], None                       # segments of one path: [path, [per-call kernel ns]]
    for t0, t1, name in recs:
        path_of = "a8w4" if ("gemm_a8w4_kernel" in name or "rowquant_fp8_kernel" in name) else "w4" if "gemm_w4_kernel" in name else None
        if path_of is None and not ("splitk_reduce_kernel" in name and cur):
            continue
        if path_of and (cur is None or cur[0] != path_of):
            cur = [path_of, []]
            seg.append(cur)
        if "rowquant" in name or "gemm_w4_kernel" in name:
            cur[1].append(0)                  # the first kernel of a call
        cur[1][-1] += t1 - t0
    cases = [(n, N, K, M) for n, N, K in SHAPES for M in ROWS]
    assert len(seg) == 2 * len(cases), (len(seg), "segments: the trace is not one run of this tool with --windows 1")
    out = []
    for i, (n, N, K, M) in enumerate(cases):
        (p2, c2), (p8, c8) = seg[2 * i], seg[2 * i + 1]
        assert (p2, p8) == ("w4", "a8w4") and len(c2) == len(c8) == WARM + reps, (p2, p8, len(c2), len(c8))
        w4, a8 = (statistics.median(c[WARM:]) / 1e3 for c in (c2, c8))
        out.append([n, str(N), str(K), str(M), f"{w4:.1f}", f"{a8:.1f}", f"{w4 / a8:.2f}", f"{2.0 * M * N * K / a8 / 1e6:.0f}"])
    table(out, ["shape", "N", "K", "rows", "w4 kernels us", "a8w4 kernels us", "w4 / a8w4", "a8w4 Tflop/s"], markdown)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--from-trace")
    args = ap.parse_args()
    if args.from_trace:
        return from_trace(args.from_trace, args.reps, args.markdown)
    import torch

    from vllm_neuron_amd import _native as lib
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without one"
    L = lib.load_library()

    def window(launch):
        for _ in range(WARM):
            launch()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            launch()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.reps

    out = []
    for name, N, K in SHAPES:
        # random code bytes and scale bytes 119 .. 134 (2^-8 .. 2^7): the contents do not matter to a timing
        img = torch.randint(0, 256, (N * K // 2 + N * K // 32,), dtype=torch.uint8, device="cuda")
        img[N * K // 2:] = torch.randint(119, 135, (N * K // 32,), dtype=torch.uint8, device="cuda")
        scale = torch.ones(N, dtype=torch.float32, device="cuda")
        for M in ROWS:
            x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            y = torch.empty(M, N, dtype=torch.float32, device="cuda")
            call = lambda path: lib.check(L.mi_op_qlinear(x.data_ptr(), M, img.data_ptr(), scale.data_ptr(), None, N, K, 3,
                                                          y.data_ptr(), path, None))
            t = {2: [], 8: []}
            for _ in range(args.windows):
                for path in (2, 8):
                    t[path].append(window(lambda: call(path)))
            w4, a8 = statistics.median(t[2]), statistics.median(t[8])
            spread = max((max(v) - min(v)) / statistics.median(v) for v in t.values())
            out.append([name, str(N), str(K), str(M), f"{w4:.1f}", f"{a8:.1f}", f"{w4 / a8:.2f}", f"{100 * spread:.0f} %"])
    table(out, ["shape", "N", "K", "rows", "w4 call us", "a8w4 call us", "w4 / a8w4", "spread"], args.markdown)


if __name__ == "__main__":
    main()
