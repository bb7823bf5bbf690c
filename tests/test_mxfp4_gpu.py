"""MXFP4 weights (MI_W_MXFP4: e2m1 codes, one e8m0 scale per 32 consecutive K of a row) on the MI355X: the load-time
quantizer bit for bit against the rule of include/mi355x_vllm.h restated in plain torch, gemv_w4_kernel / gemm_w4_kernel
against fp64 on the dequantized weights, and a model call against a bf16 context that holds the same dequantized weights."""

import functools

import pytest
import torch

from tests.helpers import decode_inputs, prefill_inputs

gpu = pytest.mark.gpu
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def mxfp4(w):
    """The rule on the CPU: fp32 [N, K] -> (codes [N, K] uint8, scale bytes [N, K / 32] uint8, dequantized fp32 [N, K])."""
    N, K = w.shape
    blk = w.float().reshape(N, K // 32, 32)
    amax = blk.abs().amax(-1, keepdim=True)
    _, e = torch.frexp(amax)                                    # amax = m * 2^e, m in [0.5, 1): floor(log2(amax)) = e - 1
    E = torch.where(amax > 0, (e - 3).clamp(-100, 100), torch.zeros_like(e))
    a = torch.ldexp(blk, -E).abs()
    # round to nearest on the grid by its midpoints; a tie goes to the even code (0.25 -> 0, 0.75 -> 1.0, 1.25 -> 1.0, ...)
    code = ((a > 0.25).int() + (a >= 0.75).int() + (a > 1.25).int() + (a >= 1.75).int() + (a > 2.5).int() + (a >= 3.5).int()
            + (a > 5.0).int())
    code = torch.where(amax > 0, code + 8 * (blk < 0).int(), torch.zeros_like(code))
    dq = torch.ldexp(GRID[(code & 7).long()] * (1 - 2 * (code >> 3)).float(), E)
    return code.reshape(N, K).to(torch.uint8), (E + 127).reshape(N, K // 32).to(torch.uint8), dq.reshape(N, K)


@pytest.fixture(scope="module")
def lib():
    from vllm_neuron_amd import _native
    return _native


def quantize_on_device(lib, w):
    """-> (the tiled image: N K / 2 code bytes + the scale plane, scale_out [N])"""
    N, K = w.shape
    wdev = w.float().contiguous().cuda()
    tiled = torch.zeros(N * K // 2 + N * ((K + 511) // 512) * 16, dtype=torch.uint8, device="cuda")
    scale = torch.empty(N, dtype=torch.float32, device="cuda")
    lib.check(lib.load_library().mi_op_quantize_weight(wdev.data_ptr(), N, K, 3, 0, tiled.data_ptr(), scale.data_ptr(), None))
    torch.cuda.synchronize()
    return tiled, scale


@gpu
def test_quantizer_bit_exact(lib):
    torch.manual_seed(0)
    N, K = 80, 256
    w = torch.randn(N, K) * 0.05
    w[3, 32:64] = 0.0                                            # an all-zero block
    w[5, 7] = 3.0                                                # one outlier
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.9, 7.99])
    w[6, 64:96] = 0.0
    w[6, 64:82] = torch.cat([ties, -ties]) / 8                   # amax 7.99 / 8 -> E = -3: every tie, the saturation band
    w[7, 0:32] = torch.randn(32).clamp(-1, 1) * 2.0 ** -30
    w[7, 0] = 2.0 ** -30                                         # a block at amax = 2^-30
    tiled, scale = quantize_on_device(lib, w)
    out = torch.empty(N * K // 2 + N * K // 32, dtype=torch.uint8, device="cuda")
    lib.check(lib.load_library().mi_op_untile_weight(tiled.data_ptr(), N, K, 3, out.data_ptr(), None))
    torch.cuda.synchronize()
    out = out.cpu()
    packed = out[:N * K // 2].reshape(N, K // 2)
    got_codes = torch.stack([packed & 15, packed >> 4], -1).reshape(N, K)   # even k in the low nibble
    codes, sbytes, _ = mxfp4(w)
    assert torch.equal(out[N * K // 2:].reshape(N, K // 32), sbytes)
    assert torch.equal(got_codes, codes)
    assert torch.equal(scale.cpu(), torch.ones(N))


@functools.lru_cache(maxsize=None)
def quantized(lib, N, K):
    """One weight matrix per shape, quantized once: (device image, scale_out, fp64 dequantized reference)."""
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(1)) * 0.05
    return (*quantize_on_device(lib, w), mxfp4(w)[2].double())


CROSS = [(M, path, N, K) for M, path in [(1, 1), (4, 1), (16, 1), (17, 1), (32, 1), (33, 0), (129, 2), (300, 2)]
         for N, K in [(48, 128), (576, 384), (1024, 4096), (256, 14336)]]


@gpu
@pytest.mark.parametrize("M,path,N,K", CROSS + [(4, 1, 272, 28672), (32, 1, 272, 28672)])
def test_qlinear(lib, M, path, N, K):
    """One tile, three tiles (not a multiple of a batch), a second MFMA column group / a second token block holding one
    row, several K-chunks, the K split.  The products are exact: test_qlinear's tolerance of the other weight dtypes."""
    tiled, scale, wdq = quantized(lib, N, K)
    torch.manual_seed(M)
    x = torch.randn(M, K).to(torch.bfloat16)
    bias = torch.randn(N) * 0.1
    ref = x.double() @ wdq.t() + bias.double()
    y = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
    xd, bd = x.cuda(), bias.cuda()
    lib.check(lib.load_library().mi_op_qlinear(xd.data_ptr(), M, tiled.data_ptr(), scale.data_ptr(), bd.data_ptr(), N, K, 3,
                                               y.data_ptr(), path, None))
    torch.cuda.synchronize()
    err = (y.cpu().double() - ref).abs().max().item()
    tol = 2e-5 * ref.abs().max().item() + 1e-5 * (K ** 0.5)
    print(f"M {M} path {path} N {N} K {K}: max |y - fp64| = {err:.3e} (tolerance {tol:.3e})")
    assert err < tol, (err, tol)


BS, MAXLEN, NSEQ = 32, 256, 4
MB = MAXLEN // BS
NB = 1 + NSEQ * MB


def model(cfg, weights, wd, kv, artifacts=None, **over):
    from vllm_neuron_amd._native import MI_KV, MI_W, NativeModel
    kw = dict(num_layers=cfg.num_layers, hidden_size=cfg.hidden_size, num_heads=cfg.num_heads, num_kv_heads=cfg.num_kv_heads,
              head_dim=cfg.head_dim, intermediate_size=cfg.intermediate_size, vocab_size=cfg.vocab_size,
              rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta, rope_type=0, rope_factor=1.0, rope_low_freq_factor=1.0,
              rope_high_freq_factor=4.0, rope_original_max_position=0, qkv_bias=0, tie_word_embeddings=0, num_blocks=NB,
              block_size=BS, max_num_seqs=NSEQ, max_model_len=MAXLEN, weight_dtype=MI_W[wd], quant_type=1, quantize_lm_head=1,
              tp_degree=1, tp_rank=0, device_id=0, use_graphs=1, kv_cache_dtype=MI_KV[kv])
    m = NativeModel(**{**kw, **over})
    try:
        m.load_artifacts(artifacts) if artifacts else m.load_state_dict(weights)
        m.finalize()
    except Exception:
        m.close()
        raise
    return m


@gpu
@pytest.mark.parametrize("kv", ["auto", "fp8"])
def test_model_matches_bf16_context_on_dequantized_weights(kv, tmp_path):
    """The same function in another summation order (0.06 on the logits, argmax equal where the top-2 gap
    exceeds 0.15): four context encodings over scattered blocks, one a prefix hit, then 8 graph-replayed decode steps at 4 rows."""
    from oracle.paged_decoder import DecoderConfig
    from oracle.synth import make_prompts, make_weights
    cfg = DecoderConfig(num_layers=2, hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=64, intermediate_size=512,
                        vocab_size=512, rms_norm_eps=1e-5, rope_theta=10000.0)
    w = make_weights(cfg, seed=1)
    wdq = {n: (mxfp4(t)[2] if n.endswith("_proj.weight") or n == "lm_head.weight" else t) for n, t in w.items()}
    m4, m16 = model(cfg, w, "mxfp4", kv), model(cfg, wdq, "bf16", kv)
    m8 = model(cfg, w, "f8e4m3", kv)
    assert m4.kv_stats()["weight_bytes"] < m8.kv_stats()["weight_bytes"]
    m8.close()
    prompts = make_prompts(cfg.vocab_size, 0)
    blocks = [[1 + (5 * (i * MB + j)) % (NB - 1) for j in range(MB)] for i in range(NSEQ)]   # scattered: 5 is coprime to NB - 1
    blocks[3][0:2] = blocks[1][0:2]                                                          # prompt 3 hits prompt 1's two full blocks
    calls = [prefill_inputs(p, blocks[i], BS, MAXLEN, 64 if i == 3 else 0) for i, p in enumerate(prompts)]
    toks, steps, worst = [0] * NSEQ, [], 0.0
    for n, inp in enumerate(calls + [None] * 8):
        if inp is None:
            inp = decode_inputs(toks, [len(p) + n - NSEQ for p in prompts], blocks, BS, MAXLEN)
        got, ref = m4.forward(**inp), m16.forward(**inp)
        steps.append((inp, got.clone()))
        worst = max(worst, (got - ref).abs().max().item())
        assert worst < 0.06, (n, worst)
        for r in range(ref.shape[0]):
            top2 = ref[r].topk(2).values
            if top2[0] - top2[1] > 0.15:
                assert int(got[r].argmax()) == int(ref[r].argmax())
        if n < NSEQ:
            toks[n] = int(ref[0].argmax())
        else:
            toks = [int(t) for t in ref.argmax(-1)]
    print(f"kv {kv}: max |mxfp4 logits - bf16 logits on the dequantized weights| = {worst:.4f}")
    m4.save_artifacts(str(tmp_path))
    m4.close()
    m16.close()
    again = model(cfg, None, "mxfp4", kv, artifacts=str(tmp_path))
    for inp, got in steps:
        assert torch.equal(again.forward(**inp), got)
    again.close()
    with pytest.raises(ValueError, match="another model"):
        model(cfg, None, "f8e4m3", kv, artifacts=str(tmp_path))


@gpu
def test_refusals(lib):
    L = lib.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    one = torch.ones(64, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    with pytest.raises(ValueError, match="K % 128"):
        lib.check(L.mi_op_quantize_weight(p, 16, 192, 3, 0, p, one.data_ptr(), None))
    with pytest.raises(ValueError, match="K % 128"):
        lib.check(L.mi_op_qlinear(p, 4, p, one.data_ptr(), None, 16, 192, 3, p, 0, None))
    with pytest.raises(ValueError, match="force_path"):
        lib.check(L.mi_op_qlinear(p, 64, p, one.data_ptr(), None, 16, 128, 3, p, 3, None))
    from oracle.paged_decoder import DecoderConfig
    cfg = DecoderConfig(num_layers=1, hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=64, intermediate_size=512,
                        vocab_size=512, rms_norm_eps=1e-5, rope_theta=10000.0)
    with pytest.raises(ValueError, match="tp_degree"):
        model(cfg, {}, "mxfp4", "auto", tp_degree=2)


def test_loader_maps_mxfp4():
    from vllm_neuron_amd.worker import mi355x_model_loader as loader
    assert loader._QUANT_DTYPES["mxfp4"] == 3
