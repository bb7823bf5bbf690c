"""INT8 x INT8 context-encoding GEMM (gemm_a8i_kernel, v_mfma_i32_16x16x64_i8): the op against fp64, and INT8 models with
prefill_int8_activations = 1 against the oracle's weight-only INT8 statement."""

from unittest import mock

import pytest
import torch

from oracle import PagedDecoderOracle
from oracle.quant import dequantize_weight, quantize_weight
from oracle.synth import make_prompts, make_weights, zoo_config

pytestmark = pytest.mark.gpu


def qlinear_a8_i8(M, N, K, k_slices):
    from tests.test_ops_gpu import dev, quantize_on_device
    from vllm_neuron_amd import _native as lib
    torch.manual_seed(3)
    w = torch.randn(N, K) * 0.05
    x = (torch.randn(M, K) * torch.rand(M, 1) * 4).to(torch.bfloat16)
    x[1] = 0                                    # all-zero token -> scale 1
    bias = torch.randn(N) * 0.1
    tiled, scale = quantize_on_device(lib, w, "int8", "per_channel_symmetric")
    y = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
    xd, bd = dev(x), dev(bias)
    lib.check(lib.load_library().mi_op_qlinear_a8_i8(xd.data_ptr(), M, tiled.data_ptr(), scale.data_ptr(), bd.data_ptr(),
                                                     N, K, k_slices, y.data_ptr(), None))
    torch.cuda.synchronize()
    return w, x, bias, y.cpu()


@pytest.mark.parametrize("M,N,K,k_slices", [(17, 16, 128, 0),        # one row past the GEMV boundary, one n-tile, one K-step
                                            (129, 272, 512, 0),      # ragged token block and ragged weight-row block
                                            (129, 272, 512, 4),      # one K-step per slice
                                            (200, 1024, 1408, 3)])   # 11 K-steps over 3 slices: ragged last slice
def test_qlinear_int8_activations(M, N, K, k_slices):
    """The activation rule restated in fp32 (s = amax / 127, all-zero row s = 1, round-half-even of x / s clamped to +-127);
    the integer sum is exact, so what remains is the fp32 scaling and the order of the slab sum."""
    w, x, bias, y = qlinear_a8_i8(M, N, K, k_slices)
    wq = dequantize_weight(*quantize_weight(w, "int8", "per_channel_symmetric"))
    xf = x.float()
    amax = xf.abs().amax(1, keepdim=True)
    s = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    xq = torch.round(xf / s).clamp(-127, 127) * s
    ref = xq.double() @ wq.double().t() + bias.double()
    err = (y.double() - ref).abs().max().item()
    tol = 2e-5 * ref.abs().max().item() + 1e-5 * (K ** 0.5)
    print(f"int8 x int8 ({M}, {N}, {K}, {k_slices}): err {err:.3e} tol {tol:.3e}")
    assert err < tol, (err, tol)


def test_qlinear_int8_activations_refuses_unsupported_k():
    with pytest.raises(ValueError):
        qlinear_a8_i8(32, 64, 192, 0)


@pytest.mark.parametrize("name", ["llama31_like", "qwen25_like"])
def test_prefill_int8_activations_matches_oracle(name):
    """The bars of test_prefill_fp8_activations_matches_oracle (8-bit activations on the same models): 0.15 on the logits,
    ids where the oracle's gap > 0.3.  qwen25_like (hidden 448) mixes both paths: only down_proj (K = 512) is served."""
    import vllm_neuron_amd._native as N
    from tests.test_model_gpu import BS, NB, load_golden, native_model, scenario
    cfg = zoo_config(name)
    w = make_weights(cfg, seed=1)
    gen, _, _ = load_golden(name)
    prompts = make_prompts(cfg.vocab_size, 0)
    quant = dict(quantized=True, quantization_dtype="int8", quantization_type="per_channel_symmetric")
    oracle = PagedDecoderOracle(cfg, w, NB, BS, compute="bf16", quant=quant)
    off = native_model(cfg, w, "int8", "per_channel_symmetric")
    orig = N.NativeModel
    with mock.patch.object(N, "NativeModel", lambda **kw: orig(prefill_int8_activations=1, **kw)):
        on = native_model(cfg, w, "int8", "per_channel_symmetric")
    worst = moved = 0.0
    for kind, inp, rows in scenario(prompts, gen):
        got, base, ref = on.forward(**inp).clone(), off.forward(**inp).clone(), oracle.forward(**inp)
        if kind == "prefill":
            moved = max(moved, (got - base).abs().max().item())
        for r in range(len(rows)):
            worst = max(worst, (got[r] - ref[r]).abs().max().item())
            top2 = ref[r].topk(2).values
            if top2[0] - top2[1] > 0.3:
                assert int(got[r].argmax()) == int(ref[r].argmax()), (kind, rows[r])
    on.close()
    off.close()
    print(f"int8 activations, {name}: worst |logits - oracle| {worst:.4f}, prefill moved by {moved:.4f}")
    assert worst < 0.15, worst
    assert moved > 0, "no prefill logit differs from the option-off model: the INT8-activation path was not taken"
