"""FP8 activations on MXFP4 weights (gemm_a8w4_kernel: the stored code tiles and e8m0 scale words as the FP4 operand and the
block scales of v_mfma_scale_f32_16x16x128_f8f6f4): the op against fp64 on the quantized operands, its refusals, and a
context with prefill_fp8_activations = 1 against the oracle's statement of the same rule on the dequantized weights."""

import functools

import pytest
import torch

from tests.helpers import decode_inputs, prefill_inputs
from tests.test_mxfp4_gpu import BS, MAXLEN, MB, NB, model, mxfp4, quantize_on_device

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from vllm_neuron_amd import _native
    return _native


@functools.lru_cache(maxsize=None)
def quantized(lib, N, K):
    """One weight matrix per shape: the block exponent moves per (row, 32-k block), so that neighbouring lanes, k-tiles and
    rows carry different scale bytes.  -> (device image, scale_out, fp64 dequantized reference)"""
    g = torch.Generator().manual_seed(1)
    w = torch.randn(N, K // 32, 32, generator=g) * 0.05 * 2.0 ** torch.randint(-4, 4, (N, K // 32, 1), generator=g)
    w = w.reshape(N, K)
    return (*quantize_on_device(lib, w), mxfp4(w)[2].double())


CASES = [(M, 8, N, K) for M in (17, 128, 129, 300) for N, K in [(48, 128), (576, 384), (1024, 4096), (256, 14336)]]
CASES += [(129, path, N, K) for path in (9, 10) for N, K in [(272, 1536), (256, 14336)]]


@gpu
@pytest.mark.parametrize("M,path,N,K", CASES)
def test_qlinear_fp8_activations_on_fp4_codes(lib, M, path, N, K):
    """One K-step, a partial scale word (KT = 3), several K-batches, the K-split's ground; a token block holding one row;
    forced 2 / 4 K-slices, ragged (8 and 4 k-tiles at K = 1536, where 4 slices are refused: 3 scale words).  Every product
    is exact in fp32: the tolerance of the exact-product GEMMs."""
    tiled, scale, wdq = quantized(lib, N, K)
    torch.manual_seed(M)
    x = (torch.randn(M, K) * torch.rand(M, 1) * 4).to(torch.bfloat16)
    x[1] = 0                                    # all-zero token -> scale 1
    bias = torch.randn(N) * 0.1
    xf = x.float()
    amax = xf.abs().amax(1, keepdim=True)
    s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    xq = (xf / s).clamp(-448, 448).to(torch.float8_e4m3fn).float() * s
    ref = xq.double() @ wdq.t() + bias.double()
    y = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
    xd, bd = x.cuda(), bias.cuda()
    run = lambda: lib.check(lib.load_library().mi_op_qlinear(xd.data_ptr(), M, tiled.data_ptr(), scale.data_ptr(), bd.data_ptr(),
                                                             N, K, 3, y.data_ptr(), path, None))
    if -(-K // 512) < {8: 1, 9: 2, 10: 4}[path]:   # the header's rule: K-slices are whole scale words (4 at K = 1536: three words)
        with pytest.raises(ValueError, match="force_path"):
            run()
        return
    run()
    torch.cuda.synchronize()
    err = (y.cpu().double() - ref).abs().max().item()
    tol = 2e-5 * ref.abs().max().item() + 1e-5 * (K ** 0.5)
    print(f"M {M} path {path} N {N} K {K}: max |y - fp64| = {err:.3e} (tolerance {tol:.3e})")
    assert err < tol, (err, tol)


@gpu
def test_refusals(lib):
    L = lib.load_library()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    one = torch.ones(64, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    with pytest.raises(ValueError, match="force_path"):
        lib.check(L.mi_op_qlinear(p, 64, p, one.data_ptr(), None, 16, 128, 1, p, 8, None))
    with pytest.raises(ValueError):
        lib.check(L.mi_op_qlinear(p, 64, p, one.data_ptr(), None, 16, 1024, 3, p, 10, None))


@gpu
@pytest.mark.parametrize("kv", ["auto", "fp8"])
def test_model_prefill_fp8_activations_matches_oracle(kv):
    """Two context encodings of more than 32 new tokens (79; 76 behind a 64-token prefix hit), then 4 decode steps at 2
    rows, which keep the GEMV on both sides.  Bars of test_prefill_fp8_activations_matches_oracle.  A context with the
    flag 0 must answer a context encoding differently: the flag is not ignored."""
    from oracle.paged_decoder import DecoderConfig, PagedDecoderOracle
    from oracle.synth import make_prompts, make_weights
    cfg = DecoderConfig(num_layers=2, hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=64, intermediate_size=512,
                        vocab_size=512, rms_norm_eps=1e-5, rope_theta=10000.0)
    w = make_weights(cfg, seed=1)
    wdq = {n: (mxfp4(t)[2] if n.endswith("_proj.weight") or n == "lm_head.weight" else t) for n, t in w.items()}
    oracle = PagedDecoderOracle(cfg, wdq, NB, BS, compute="bf16", prefill_fp8_activations=True)
    oracle.a8_weights = {n for n in w if n.endswith("_proj.weight")}
    m8, m0 = model(cfg, w, "mxfp4", kv, prefill_fp8_activations=1), model(cfg, w, "mxfp4", kv)
    prompts = [make_prompts(cfg.vocab_size, 0)[i] for i in (1, 3)]          # 79 and 140 tokens, 64 shared
    blocks = [[1 + (5 * (i * MB + j)) % (NB - 1) for j in range(MB)] for i in range(2)]
    blocks[1][0:2] = blocks[0][0:2]
    calls = [prefill_inputs(p, blocks[i], BS, MAXLEN, 64 * i) for i, p in enumerate(prompts)]
    toks, worst = [0, 0], 0.0
    for n, inp in enumerate(calls + [None] * 4):
        if inp is None:
            inp = decode_inputs(toks, [len(p) + n - 2 for p in prompts], blocks, BS, MAXLEN)
        got, ref = m8.forward(**inp), oracle.forward(**inp)
        if n < 2:
            assert not torch.equal(got, m0.forward(**inp)), "prefill_fp8_activations changed nothing"
        worst = max(worst, (got - ref).abs().max().item())
        for r in range(ref.shape[0]):
            top2 = ref[r].topk(2).values
            if top2[0] - top2[1] > 0.3:
                assert int(got[r].argmax()) == int(ref[r].argmax()), (n, r)
        if n < 2:
            toks[n] = int(ref[0].argmax())
        else:
            toks = [int(t) for t in ref.argmax(-1)]
    print(f"kv {kv}: max |device logits - oracle logits| = {worst:.4f}")
    assert worst < 0.15, worst
    m8.close()
    m0.close()
